"""The cases of tests/golden/twin_bits.npz: the twin's outputs, pinned as raw 64-bit patterns.

Four lanes, one per shape, K = 3 SQP iterations, a cold and then a warm controller step, at the
smallest horizons that reach each path of the arithmetic the twin shares with the kernels
(csrc/qsp_fp.hpp, qsp_math.hpp, qsp_riccati.hpp, qsp_ipm.hpp).  tests/golden/make_twin_bits.py
writes the fixture from these, tests/test_twin_bits.py compares against it.
"""
import ctypes as C

import numpy as np

from oracle.oracle import Oracle, make_opts
from qp_data import build_qp

NAMES = ("santal", "balea", "montana", "pulirapid")
K = 3

# name -> make_opts arguments, plus: "loop": helper.closed_loop_matlab instead of controller steps
# ("dist": with a disturbance and its contact re-projection); "s_out": lane 1 starts with its contact
# coordinate above uh_s; "kkt": the merit SQP's 8 diagnostics per lane too; "qp": the QP alone
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
}


def inputs():
    rng = np.random.default_rng(20261020)
    B = len(NAMES)
    x0 = np.stack([rng.uniform(-0.0065, 0.0260, B), rng.uniform(-0.0197, 0.0124, B),
                   np.deg2rad(rng.uniform(-8.05, 9.30, B)), rng.uniform(-0.0382, 0.0011, B)], 1)
    t = np.arange(0.0, 10.0 + 1e-9, 0.05)
    traj = np.zeros((len(t), 6))
    traj[:, 0] = 0.01 * t
    return x0, traj, np.arange(B, dtype=np.int32)


def qp_inputs(tw, op, x0, traj, sid):
    """The Gauss-Newton QP of a perturbed iterate around x0 (qp_data.build_qp), seeded."""
    rng = np.random.default_rng(20261020 + op.N)
    B, N = len(x0), op.N
    X = np.repeat(x0[:, None], N + 1, 1) + rng.normal(0, 2e-3, (B, N + 1, 4))
    U = np.stack([rng.uniform(0, 0.03, (B, N)), rng.uniform(-0.02, 0.02, (B, N))], 2)
    yref = np.broadcast_to(traj[None, :N], (B, N, 6)).copy()
    A, Bm, b, H, g, lo, hi, act, dx0 = build_qp(tw, op, X, U, yref, yref[:, -1, :4], x0, sid)
    return A.reshape(B, N, 16), Bm.reshape(B, N, 8), b, H, g, lo, hi, act, dx0


def run_cases():
    """{"<case>/<step>/<array>": ndarray} of every case, from the twin as built."""
    from uclv_qs_pushing_matlab_amd.objects import object_selection
    tw = Oracle(NAMES, twin=True)
    x0, traj, sid = inputs()
    out = {}
    for name, kw in CASES.items():
        kw = dict(kw)
        loop, dist, s_out, kkt, qp = (kw.pop(f, False) for f in ("loop", "dist", "s_out", "kkt", "qp"))
        op = make_opts(**{"sqp_iters": K, **kw})
        if loop:
            extra = {}
            if dist:
                extra = dict(dist_step=3, dist_amp=np.array([0.003, -0.004, 0.002, -0.0025]),
                             xwidth=np.array([object_selection(n)["xwidth"] for n in NAMES]))
            r = tw.closed_loop(op, x0, traj, 5, shape_id=sid, delay_cols=2, plant_delay_cols=2, **extra)
            for k in ("X", "Xsim", "U", "status"):
                out[f"{name}/loop/{k}"] = r[k]
            continue
        if qp:
            r = tw.qp(op, *qp_inputs(tw, op, x0, traj, sid))
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
