"""The cases of tests/golden/twin_bits.npz: the twin's outputs, pinned as raw 64-bit patterns.

Four lanes, one per shape, K = 3 SQP iterations, a cold and then a warm controller step, at the
smallest horizons that reach each path of the arithmetic the twin shares with the kernels
(csrc/qsp_fp.hpp, qsp_math.hpp, qsp_riccati.hpp, qsp_ipm.hpp), and of the per-lane code around the solve
that it shares with them too: the staging's delay prefix and end clamp on a per-lane table, the acados-level
solve, the closed loop with noise, a seeded controller buffer and a plant without delay, the building blocks'
output layout, the QP-level statuses 2 and 3.  tests/golden/make_twin_bits.py
writes the fixture from these, tests/test_twin_bits.py compares against it.
"""
import ctypes as C

import numpy as np

from oracle.oracle import Oracle, make_opts
from qp_data import build_qp

NAMES = ("santal", "balea", "montana", "pulirapid")
K = 3

# name -> make_opts arguments, plus: "loop": helper.closed_loop_matlab instead of controller steps
# ("dist": with a disturbance and its contact re-projection; "noise": sim_noise, a non-zero initial
# controller buffer and a plant without delay); "s_out": lane 1 starts with its contact coordinate above
# uh_s; "kkt": the merit SQP's 8 diagnostics per lane too; "qp": the QP alone ("s0_out": lane 1's dx0 s
# above hi of stage 0); "edges": cold controller steps on the per-lane table of delay_edge_table, in its
# delay prefix and past its end; "ocp": the acados-level solve; "blocks": the building blocks
CASES = {
    "s1_n5_lane": dict(N=5),                                                # S = 1, lane walk
    "s1_n12_mfma": dict(N=12),                                              # S = 1, matrix-core order
    "s1_n12_lane": dict(N=12, lane_walk=1),                                 # S = 1, lane walk at N = 12
    "s2_n9_lane": dict(N=9, stages_per_lane=2),                             # S = 2, lane walk
    "s2_n24_mfma": dict(N=24, stages_per_lane=2),                           # S = 2, matrix-core order
    "s2_n24_scan": dict(N=24, stages_per_lane=2, factor_scan=1),            # S = 2, factorisation scan
    "merit_n12": dict(N=12, nlp_mode=1),                                    # merit SQP
    "loop_n12_delay": dict(N=12, loop=True),                                # closed loop, delay compensation
    "s1_n5_nos0": dict(N=5, stage0_s_bound=0),                              # no bound on stage 0's s
    "s2_n9_nos0": dict(N=9, stages_per_lane=2, stage0_s_bound=0),           # the same at S = 2
    "s1_n5_s0_infeasible": dict(N=5, s_out=True),                           # one lane refused (status 4)
    "merit_n12_long": dict(N=12, nlp_mode=1, sqp_iters=30, kkt=True),       # merit SQP to its end: status 0 and 2
    "loop_n12_dist": dict(N=12, loop=True, dist=True),                      # closed loop with a disturbance
    "qp_n5": dict(N=5, qp=True),                                            # the QP alone, S = 1
    "qp_n9_s2": dict(N=9, stages_per_lane=2, qp=True),                      # the QP alone, S = 2
    "qp_n5_stall": dict(N=5, qp=True, qp_stall_alpha=0.9, qp_stall_iters=2),  # two lanes leave by the stall exit (status 4)
    "ctrl_n5_delay_edges": dict(N=5, edges=True),                           # staging: delay prefix, end clamp, per-lane table
    "ocp_n5": dict(N=5, sqp_iters=4, ocp=True),                             # acados-level solve: unshifted outputs
    "ocp_merit_n5": dict(N=5, sqp_iters=4, nlp_mode=1, ocp=True),           # ... and nlp_mode 1's PI and lam (status 2)
    "loop_n5_noise": dict(N=5, loop=True, noise=True),                      # noise, seeded buffer, plant without delay
    "blocks": dict(blocks=True),                                            # building blocks' output packing
    "qp_n5_cap": dict(N=5, qp=True, qp_iters=3),                            # every lane leaves at the cap (qp_status 2)
    "qp_n5_s0_out": dict(N=5, qp=True, s0_out=True),                        # lane 1 infeasible at stage 0 (qp_status 3)
}
EDGE_T, EDGE_DELAY_COLS = 8, 2


def inputs():
    rng = np.random.default_rng(20261020)
    B = len(NAMES)
    x0 = np.stack([rng.uniform(-0.0065, 0.0260, B), rng.uniform(-0.0197, 0.0124, B),
                   np.deg2rad(rng.uniform(-8.05, 9.30, B)), rng.uniform(-0.0382, 0.0011, B)], 1)
    t = np.arange(0.0, 10.0 + 1e-9, 0.05)
    traj = np.zeros((len(t), 6))
    traj[:, 0] = 0.01 * t
    return x0, traj, np.arange(B, dtype=np.int32)


def delay_edge_table():
    """ctrl_n5_delay_edges' reference: one table of EDGE_T rows per lane, each lane's its own (another
    speed, a y drift, its own s_ref and a non-zero u_t reference, which the delay prefix copies)."""
    t = 0.05 * np.arange(EDGE_T)
    tab = np.zeros((len(NAMES), EDGE_T, 6))
    for i in range(len(NAMES)):
        tab[i, :, 0] = (0.01 + 0.002 * i) * t
        tab[i, :, 1] = -0.001 * i * t
        tab[i, :, 3] = -0.002 * i
        tab[i, :, 5] = 0.002 * (i + 1) * (1.0 + t)
    return tab


def edge_index_times():
    return (1, EDGE_T, EDGE_T + 4)


def block_points():
    """8 seeded points per shape for the building blocks, among them u = (0, 0) and u_n = 0."""
    rng = np.random.default_rng(20261021)
    n = 8 * len(NAMES)
    sid = np.repeat(np.arange(len(NAMES), dtype=np.int32), 8)
    x = np.stack([rng.uniform(-0.01, 0.03, n), rng.uniform(-0.02, 0.02, n), rng.uniform(-0.2, 0.2, n),
                  rng.uniform(-0.04, 0.01, n)], 1)
    u = np.stack([rng.uniform(0.0, 0.03, n), rng.uniform(-0.05, 0.05, n)], 1)
    u[0::8] = 0.0
    u[1::8, 0] = 0.0
    return x, u, sid


def qp_inputs(tw, op, x0, traj, sid, s0_out=False):
    """The Gauss-Newton QP of a perturbed iterate around x0 (qp_data.build_qp), seeded."""
    rng = np.random.default_rng(20261020 + op.N)
    B, N = len(x0), op.N
    X = np.repeat(x0[:, None], N + 1, 1) + rng.normal(0, 2e-3, (B, N + 1, 4))
    U = np.stack([rng.uniform(0, 0.03, (B, N)), rng.uniform(-0.02, 0.02, (B, N))], 2)
    yref = np.broadcast_to(traj[None, :N], (B, N, 6)).copy()
    A, Bm, b, H, g, lo, hi, act, dx0 = build_qp(tw, op, X, U, yref, yref[:, -1, :4], x0, sid)
    if s0_out:
        dx0[1, 3] = hi[1, 0, 0] + 0.001          # lane 1's dx0 s above hi of stage 0
    return A.reshape(B, N, 16), Bm.reshape(B, N, 8), b, H, g, lo, hi, act, dx0


def run_cases():
    """{"<case>/<step>/<array>": ndarray} of every case, from the twin as built."""
    from uclv_qs_pushing_matlab_amd.objects import object_selection
    tw = Oracle(NAMES, twin=True)
    x0, traj, sid = inputs()
    out = {}
    for name, kw in CASES.items():
        kw = dict(kw)
        loop, dist, s_out, kkt, qp, noise, s0_out, edges, ocp, blocks = (kw.pop(f, False) for f in (
            "loop", "dist", "s_out", "kkt", "qp", "noise", "s0_out", "edges", "ocp", "blocks"))
        op = make_opts(**{"sqp_iters": K, **kw})
        if blocks:
            x, u, bsid = block_points()
            r = dict(zip(("C", "D", "Dd", "kappa"), tw.spline(x[:, 3], bsid)))
            r["f"], r["J"] = tw.dynamics(x, u, bsid)
            r["xn"], r["A"], r["B"] = tw.rk4(x, u, op.Ts, bsid)
            r["vb"] = tw.vbound(x[:, 3], op, bsid)
            for k, v in r.items():
                out[f"{name}/blocks/{k}"] = v
            continue
        if edges:
            for it in edge_index_times():        # every step cold
                warm = tw.new_warm(len(x0), op.N)
                r = tw.controller_solve(op, x0, delay_edge_table(), it, warm, shape_id=sid, delay_cols=EDGE_DELAY_COLS)
                for k in ("u0", "status", "iters", "qp_iter", "cost"):
                    out[f"{name}/{it}/{k}"] = r[k]
                for k in ("X", "U", "PI"):
                    out[f"{name}/{it}/{k}"] = warm[k]
            continue
        if ocp:
            B, N = len(x0), op.N
            r = tw.ocp_solve(op, x0, traj[:N], traj[N - 1, :4], X=np.repeat(x0[:, None], N + 1, 1),
                             U=np.tile([0.01, 0.002], (B, N, 1)), shape_id=sid)
            for k in ("X", "U", "PI", "lam", "status", "iters", "cost"):
                out[f"{name}/ocp/{k}"] = r[k]
            continue
        if loop:
            extra = dict(delay_cols=2, plant_delay_cols=2)
            if dist:
                extra.update(dist_step=3, dist_amp=np.array([0.003, -0.004, 0.002, -0.0025]),
                             xwidth=np.array([object_selection(n)["xwidth"] for n in NAMES]))
            if noise:
                rng = np.random.default_rng(20261022)
                extra = dict(delay_cols=1, plant_delay_cols=0,
                             noise=rng.standard_normal((4, len(x0), 4)) * np.array([1e-5, 1e-5, 1e-3, 1e-4]),
                             ubc0=np.stack([rng.uniform(0.0, 0.03, (len(x0), 1)), rng.uniform(-0.02, 0.02, (len(x0), 1))], 2))
            r = tw.closed_loop(op, x0, traj, 4 if noise else 5, shape_id=sid, **extra)
            for k in ("X", "Xsim", "U", "status"):
                out[f"{name}/loop/{k}"] = r[k]
            continue
        if qp:
            r = tw.qp(op, *qp_inputs(tw, op, x0, traj, sid, s0_out))
            for k in ("dx", "du", "lam", "iters", "qp_status"):
                out[f"{name}/qp/{k}"] = r[k]
            continue
        warm = tw.new_warm(len(x0), op.N)
        x = x0.copy()
        if s_out:
            x[1, 3] = 0.02                       # above uh_s = 0.011
        diag = np.zeros((len(x0), 8))
        if kkt:
            tw.L.tw_set_kkt_diag(diag.ctypes.data_as(C.c_void_p))
        try:
            for step in (1, 2):                  # cold start, then the shifted warm start
                r = tw.controller_solve(op, x, traj, step, warm, shape_id=sid)
                for k in ("u0", "status", "qp_iter", "cost"):
                    out[f"{name}/{step}/{k}"] = r[k].copy()
                for k in ("X", "U", "PI"):
                    out[f"{name}/{step}/{k}"] = warm[k].copy()
                if s_out or kkt:
                    out[f"{name}/{step}/sqp_iter"] = r["iters"].copy()
                if kkt:
                    out[f"{name}/{step}/kkt"] = diag.copy()
                f, _ = tw.dynamics(x, r["u0"], sid)
                x = x + 0.05 * f
        finally:
            if kkt:                              # a process-global pointer: clear it on every exit path
                tw.L.tw_set_kkt_diag(None)
    return out


def as_bits(a):
    """The array's raw bit patterns (doubles as uint64; integer arrays as they are)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a
