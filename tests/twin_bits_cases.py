"""The cases of tests/golden/twin_bits.npz: the twin's outputs, pinned as raw 64-bit patterns.

Four lanes, one per shape, K = 3 SQP iterations, a cold and then a warm controller step, at the
smallest horizons that reach each path of the arithmetic the twin shares with the kernels
(csrc/qsp_fp.hpp, qsp_math.hpp, qsp_riccati.hpp).  tests/golden/make_twin_bits.py writes the
fixture from these, tests/test_twin_bits.py compares against it.
"""
import numpy as np

from oracle.oracle import Oracle, make_opts

NAMES = ("santal", "balea", "montana", "pulirapid")
K = 3

# name -> make_opts arguments; "loop": helper.closed_loop_matlab instead of controller steps
CASES = {
    "s1_n5_lane": dict(N=5),                                                # S = 1, lane walk
    "s1_n12_mfma": dict(N=12),                                              # S = 1, matrix-core order
    "s1_n12_lane": dict(N=12, lane_walk=1),                                 # S = 1, lane walk at N = 12
    "s2_n9_lane": dict(N=9, stages_per_lane=2),                             # S = 2, lane walk
    "s2_n24_mfma": dict(N=24, stages_per_lane=2),                           # S = 2, matrix-core order
    "s2_n24_scan": dict(N=24, stages_per_lane=2, factor_scan=1),            # S = 2, factorisation scan
    "merit_n12": dict(N=12, nlp_mode=1),                                    # merit SQP
    "loop_n12_delay": dict(N=12, loop=True),                                # closed loop, delay compensation
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


def run_cases():
    """{"<case>/<step>/<array>": ndarray} of every case, from the twin as built."""
    tw = Oracle(NAMES, twin=True)
    x0, traj, sid = inputs()
    out = {}
    for name, kw in CASES.items():
        kw = dict(kw)
        loop = kw.pop("loop", False)
        op = make_opts(sqp_iters=K, **kw)
        if loop:
            r = tw.closed_loop(op, x0, traj, 5, shape_id=sid, delay_cols=2, plant_delay_cols=2)
            for k in ("X", "Xsim", "U", "status"):
                out[f"{name}/loop/{k}"] = r[k]
            continue
        warm = tw.new_warm(len(x0), op.N)
        x = x0.copy()
        for step in (1, 2):                      # cold start, then the shifted warm start
            r = tw.controller_solve(op, x, traj, step, warm, shape_id=sid)
            for k in ("u0", "status", "qp_iter", "cost"):
                out[f"{name}/{step}/{k}"] = r[k].copy()
            for k in ("X", "U", "PI"):
                out[f"{name}/{step}/{k}"] = warm[k].copy()
            f, _ = tw.dynamics(x, r["u0"], sid)
            x = x + 0.05 * f
    return out


def as_bits(a):
    """The array's raw bit patterns (doubles as uint64; integer arrays as they are)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a
