"""numpy restatement of qsp_closed_loop_metrics (include/qsp_nmpc.h, QSP_CLM_*), applied to a closed loop's
trajectories: the reference the device accumulators are compared with bit for bit.

One accumulator per metric, updated in step order with the products and sums the header spells out
(e_x * e_x + e_y * e_y, then acc + that); every operation is one IEEE double operation per lane on both sides.
"""
import numpy as np

NAMES = ("sum_exy2", "max_exy2", "sum_eth2", "end_exy2", "sum_u2", "n_failed", "n_st", "n_sl", "n_sr", "n_s_out")


def ref_rows(traj, index0, col, B):
    """Rows of the reference table at the 1-based columns index0 + col per lane, clamped into the table as
    get_y_ref clamps (NMPC_controller.m:307-313).  traj (T, 6) shared or (B, T, 6) per lane -> (B, 6)."""
    traj = np.asarray(traj, np.float64)
    T = traj.shape[-2]
    c = np.clip(np.broadcast_to(np.asarray(index0, np.int64), (B,)) + col, 1, T) - 1
    return traj[c] if traj.ndim == 2 else traj[np.arange(B), c]


def closed_loop_metrics_ref(X, U, status, modes, traj, index0, s_lo, s_hi):
    """X (B, n + 1, 4) logged plant states and the final one, U (B, n, 2) commanded inputs, status (B, n),
    modes (B, n) QSP_MODE_* of the applied input at the logged state under the plant's model, traj the
    installed reference table, index0 scalar or (B,) 1-based, [s_lo, s_hi] the handle's bound on s.
    -> (B, 10) in the order of NAMES."""
    X, U = np.asarray(X, np.float64), np.asarray(U, np.float64)
    B, n = U.shape[:2]
    m = np.zeros((B, len(NAMES)))
    for t in range(n):
        r = ref_rows(traj, index0, t, B)
        ex, ey, et = X[:, t, 0] - r[:, 0], X[:, t, 1] - r[:, 1], X[:, t, 2] - r[:, 2]
        e2 = ex * ex + ey * ey
        m[:, 0] = m[:, 0] + e2
        m[:, 1] = np.where(e2 > m[:, 1], e2, m[:, 1])
        m[:, 2] = m[:, 2] + et * et
        m[:, 4] = m[:, 4] + (U[:, t, 0] * U[:, t, 0] + U[:, t, 1] * U[:, t, 1])
        m[:, 5] = m[:, 5] + (np.asarray(status)[:, t] != 0)
        for k in (1, 2, 3):                       # ST, SL, SR; mode 0 is counted nowhere
            m[:, 5 + k] = m[:, 5 + k] + (np.asarray(modes)[:, t] == k)
        s = X[:, t, 3]
        m[:, 9] = m[:, 9] + ~((s >= s_lo) & (s <= s_hi))
    r = ref_rows(traj, index0, n, B)
    fx, fy = X[:, n, 0] - r[:, 0], X[:, n, 1] - r[:, 1]
    m[:, 3] = fx * fx + fy * fy
    return m
