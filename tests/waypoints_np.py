"""numpy restatement of qsp_gen_waypoints (include/qsp_nmpc.h), every operation written out in the order the
library takes it, so that the device table can be held to it bit for bit: the host preparation of
qsp_capi.hip (segment durations, arrival times or row counts, headings) and the row rule of waypoints_kernel.
Shared by tests/test_waypoints.py and tests/test_gpu_waypoints.py; no test of its own."""
import numpy as np

LAWS = ("constant_speed", "segment_linspace")
YAWS = ("heading", "heading_unwrapped", "fixed")

# the reference's paths
MAIN_TWO = np.array([[0.0, 0.0], [0.10, 0.0]])                                                   # main.m:150-161
DISTURBANCE = np.array([[0.0, 0.0], [0.20, 0.0], [0.20, 0.05], [0.20, 0.15], [0.20, 0.20], [0.0, 0.20]])  # :132-139
THREE_SEGMENT = np.array([[0.0, 0.0], [0.12, 0.0], [0.12, 0.06], [0.12, 0.12]])                  # :141-148


def segments(wp, vel):
    """Durations d_k and headings h_k of one lane's segments: wp (n, 2), vel (n - 1,)."""
    dx = wp[1:, 0] - wp[:-1, 0]
    dy = wp[1:, 1] - wp[:-1, 1]
    return np.sqrt(dx * dx + dy * dy) / vel, np.arctan2(dy, dx)


def arrival_times(d):
    return np.concatenate([[0.0], np.cumsum(d)])      # t_0 = 0, t_{k+1} = t_k + d_k, in sequence


def segment_yaw(h, yaw, theta):
    if yaw == "fixed":
        return np.full(len(h), float(theta))
    if yaw == "heading":
        return h.copy()
    y = h.copy()
    for k in range(1, len(h)):
        dl = h[k] - h[k - 1]
        dl = dl - 2 * np.pi * np.rint(dl / (2 * np.pi))
        y[k] = y[k - 1] + dl
    return y


def lane_rows(wp, vel, Ts, law="constant_speed", yaw="heading", theta=None, s_ref=0.0):
    """One lane's T_i x 6 rows [x y yaw s_ref 0 0]."""
    wp = np.asarray(wp, np.float64)
    n = len(wp)
    vel = np.broadcast_to(np.asarray(vel, np.float64), (n - 1,))
    d, h = segments(wp, vel)
    ys = segment_yaw(h, yaw, theta)
    if law == "constant_speed":
        t = arrival_times(d)
        Ti = int(np.floor(t[-1] / Ts + 1e-9)) + 1
        tt = np.arange(Ti).astype(np.float64) * Ts                                     # j*Ts, one product
        k = np.minimum(np.searchsorted(t, tt, side="right") - 1, n - 2)                # last k with t_k <= t, capped
        a = (tt - t[k]) / (t[k + 1] - t[k])
        x = wp[k, 0] + a * (wp[k + 1, 0] - wp[k, 0])
        y = wp[k, 1] + a * (wp[k + 1, 1] - wp[k, 1])
        seg = k
    else:
        x, y, seg = [wp[0, 0]], [wp[0, 1]], [0]
        for k in range(n - 1):
            nk = int(np.floor(d[k] / Ts + 1e-9))
            for m in range(nk):
                if m == nk - 1:
                    x.append(wp[k + 1, 0])
                    y.append(wp[k + 1, 1])
                else:
                    x.append(wp[k, 0] + m * ((wp[k + 1, 0] - wp[k, 0]) / (nk - 1)))
                    y.append(wp[k, 1] + m * ((wp[k + 1, 1] - wp[k, 1]) / (nk - 1)))
                seg.append(k)
        x, y, seg = np.array(x), np.array(y), np.array(seg)
    rows = np.zeros((len(x), 6))
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = x, y, ys[seg], s_ref
    return rows


def table(wp, vel, Ts, n_wp=None, law="constant_speed", yaw="heading", theta=None, s_ref=None):
    """The installed table: wp (B, K, 2), vel (B, K - 1) -> T, T_lane (B,), tab (B, T, 6); a lane with
    T_i < T repeats its last row."""
    wp = np.asarray(wp, np.float64)
    B, K = wp.shape[:2]
    vel = np.broadcast_to(np.asarray(vel, np.float64), (B, K - 1))
    n_wp = np.full(B, K) if n_wp is None else np.asarray(n_wp)
    lanes = [lane_rows(wp[i, :n_wp[i]], vel[i, :n_wp[i] - 1], Ts, law, yaw,
                       None if theta is None else np.broadcast_to(theta, (B,))[i],
                       0.0 if s_ref is None else np.broadcast_to(s_ref, (B,))[i]) for i in range(B)]
    T_lane = np.array([len(r) for r in lanes], np.int32)
    T = int(T_lane.max())
    tab = np.stack([np.concatenate([r, np.repeat(r[-1:], T - len(r), axis=0)]) for r in lanes])
    return T, T_lane, tab
