"""numpy restatement of the rollout-cost and u0-cost-landscape entry points (TEST INFRASTRUCTURE ONLY).

`helper.evaluate_cost_function` / `helper.debug_cost_function` (helper.m:356-431) with the OCP's model:
f and the RK4 step come from the CPU oracle (`Oracle.dynamics`, `Oracle.rk4`; literal restatement or
kernel-order twin), the sums are plain numpy in the device's order.  numpy has no fused multiply-add,
so against the device this is a tolerance comparison, never bit identity.
"""
import numpy as np

W = np.array([1.0, 1.0, 1e-3, 0.0, 1e-3, 1e-3])      # main.m:82-86 (x 0.01 folded), NMPC_controller.m:16-18
WE = np.array([2e5, 2e5, 20.0, 0.0])
LH = np.array([-0.06, 0.0, -0.05])                   # NMPC_controller.m:23-26, 251-252
UH = np.array([0.011, 0.03, 0.05])
TS = 0.05


def colon_grid(lb, ub, step=0.005):
    """MATLAB's lb:step:ub as lb + k step, k = 0..floor((ub - lb) / step + 1e-10) (helper.m:380-381)."""
    k = int(np.floor((ub - lb) / step + 1e-10))
    return lb + np.arange(k + 1) * step


def first_min(surface):
    """MATLAB's [m, i] = min(v(:)) per row of surface (B, G): the first minimum in linear order, NaN never
    wins, an all-NaN row gives (NaN, 0).  Returns (cost_min (B,), idx_min (B,) 0-based)."""
    s = np.asarray(surface, np.float64)
    s = s.reshape(s.shape[0], -1)
    cmin = np.full(s.shape[0], np.nan)
    imin = np.zeros(s.shape[0], np.int32)
    for b in range(s.shape[0]):
        best, ib = 0.0, -1
        for g, c in enumerate(s[b]):
            if c == c and (ib < 0 or c < best):
                best, ib = c, g
        if ib >= 0:
            cmin[b], imin[b] = best, ib
    return cmin, imin


def rollout_cost(oracle, x0, U, sid, yref, yref_e, integrator="euler", tau=TS, Ts=TS, W=W, We=WE, lh=LH, uh=UH,
                 s0_bound=True):
    """x0 (B, 4), U (B, M, N, 2), sid (B,), yref (B, N, 6), yref_e (B, 4) -> cost (B, M), viol (B, M),
    x_end (B, M, 4).  tau: the stage-cost scaling (Ts for the handle's objective, 1 unscaled)."""
    U = np.asarray(U, np.float64)
    B, M, N = U.shape[:3]
    x = np.repeat(np.asarray(x0, np.float64)[:, None], M, 1).reshape(B * M, 4)
    sidf = np.repeat(np.asarray(sid, np.int32), M)
    yr = np.repeat(np.asarray(yref, np.float64)[:, None], M, 1).reshape(B * M, N, 6)
    ye = np.repeat(np.asarray(yref_e, np.float64)[:, None], M, 1).reshape(B * M, 4)
    Uf = U.reshape(B * M, N, 2)
    cost = np.zeros(B * M)
    viol = np.zeros(B * M)
    for k in range(N):
        u = Uf[:, k]
        e = np.concatenate([x, u], 1) - yr[:, k]
        s = np.zeros(B * M)
        for q in range(6):
            s = W[q] * e[:, q] * e[:, q] + s
        cost = 0.5 * tau * s + cost
        v = np.stack([x[:, 3], u[:, 0], u[:, 1]], 1)
        for j in range(3):
            if j == 0 and k == 0 and not s0_bound:
                continue
            vl, vh = lh[j] - v[:, j], v[:, j] - uh[j]
            viol = np.where(vl > viol, vl, viol)
            viol = np.where(vh > viol, vh, viol)
        if integrator == "rk4":
            x = oracle.rk4(x, u, Ts, sidf)[0]
        else:
            x = x + Ts * oracle.dynamics(x, u, sidf)[0]
    e = x - ye
    s = np.zeros(B * M)
    for q in range(4):
        s = We[q] * e[:, q] * e[:, q] + s
    cost = 0.5 * s + cost
    return cost.reshape(B, M), viol.reshape(B, M), x.reshape(B, M, 4)


def landscape_candidates(U_tail, un, ut):
    """(B, n_un * n_ut, N, 2): u_0 = (un[i], ut[j]) at linear index i n_ut + j, u_k = U_tail[k] for k >= 1."""
    U_tail = np.asarray(U_tail, np.float64)
    G = len(un) * len(ut)
    cand = np.repeat(U_tail[:, None], G, 1).copy()
    cand[:, :, 0, 0] = np.repeat(un, len(ut))[None]
    cand[:, :, 0, 1] = np.tile(ut, len(un))[None]
    return cand


def cost_landscape(oracle, x0, U_tail, un, ut, sid, yref, yref_e, **kw):
    """-> surface (B, n_un, n_ut), u_min (B, 2), cost_min (B,), idx_min (B,)."""
    cand = landscape_candidates(U_tail, un, ut)
    cost = rollout_cost(oracle, x0, cand, sid, yref, yref_e, **kw)[0]
    cmin, imin = first_min(cost)
    u_min = np.stack([np.asarray(un)[imin // len(ut)], np.asarray(ut)[imin % len(ut)]], 1)
    return cost.reshape(len(cost), len(un), len(ut)), u_min, cmin, imin
