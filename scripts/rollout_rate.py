"""Rate of the rollout-cost kernels on the bench batch (developer tool, needs the GPU).

Times, with HIP events on device-resident data after a warm-up and outside any copy:
  * the NULL-surface cost landscape (qsp_cost_landscape_device) at B = 65 536, N = 20, the 7 x 21 grid
    of helper.m:380-381, for both integrators;
  * qsp_rollout_cost_device at M = 147 on the same candidates, assembled in device memory;
and prints rollouts/s and stage evaluations/s next to the numpy restatement's rate (tests/rollout_ref.py
over the CPU oracle) on 64 lanes with the host's threads.

  python scripts/rollout_rate.py [--batch 65536] [--reps 5] [--no-cpu] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAMES = ("santal", "balea", "montana", "pulirapid")


def config2_x0(nb, seed):   # BASELINE config 2 initial-state law (main.m:53-56 ranges)
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-0.0065, 0.0260, nb), rng.uniform(-0.0197, 0.0124, nb),
                     np.deg2rad(rng.uniform(-8.05, 9.30, nb)), rng.uniform(-0.0382, 0.0011, nb)], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from uclv_qs_pushing_matlab_amd import _lib
    from uclv_qs_pushing_matlab_amd.objects import make_shape
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver

    B, N = a.batch, a.N
    dev = torch.device("cuda:0")
    un = np.arange(7) * 0.005                      # u_n_lb:0.005:u_n_ub
    ut = -0.05 + np.arange(21) * 0.005             # u_t_lb:0.005:u_t_ub
    G = len(un) * len(ut)
    rng = np.random.default_rng(1)
    x0 = config2_x0(B, 21)
    sid = (np.arange(B) % 4).astype(np.int32)
    tail = np.stack([rng.uniform(0.001, 0.03, (B, N)), rng.uniform(-0.05, 0.05, (B, N))], 2)
    traj = np.zeros((N, 6))
    traj[:, 0] = 0.01 * 0.05 * np.arange(N)
    yref = np.repeat(traj[None], B, 0)

    s = OcpSolver(N=N, batch=B)
    s.set_shapes([make_shape(n) for n in NAMES], shape_id=sid)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    d_x0, d_tail, d_yref, d_ye = t(x0), t(tail), t(yref), t(yref[:, N - 1, :4])
    d_un, d_ut = t(un), t(ut)
    d_umin, d_cmin = torch.zeros(B, 2, dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.float64, device=dev)
    d_imin = torch.zeros(B, dtype=torch.int32, device=dev)
    lio = _lib.LandscapeIO()
    lio.x0, lio.U_tail, lio.un_grid, lio.ut_grid = d_x0.data_ptr(), d_tail.data_ptr(), d_un.data_ptr(), d_ut.data_ptr()
    lio.yref, lio.yref_e = d_yref.data_ptr(), d_ye.data_ptr()
    lio.u_min, lio.cost_min, lio.idx_min = d_umin.data_ptr(), d_cmin.data_ptr(), d_imin.data_ptr()
    lio.n_un, lio.n_ut = len(un), len(ut)
    # the same candidates assembled in device memory (B x G x N x 2)
    d_U = d_tail[:, None].repeat(1, G, 1, 1)
    d_U[:, :, 0, 0] = d_un.repeat_interleave(len(ut))[None]
    d_U[:, :, 0, 1] = d_ut.repeat(len(un))[None]
    d_cost = torch.zeros(B, G, dtype=torch.float64, device=dev)
    rio = _lib.RolloutIO()
    rio.x0, rio.U, rio.yref, rio.yref_e, rio.cost = (d_x0.data_ptr(), d_U.data_ptr(), d_yref.data_ptr(), d_ye.data_ptr(),
                                                     d_cost.data_ptr())
    # a stream of our own: the events and the launches must share it (a NULL stream argument would mean
    # the handle's stream)
    tstream = torch.cuda.Stream()
    torch.cuda.synchronize()
    torch.cuda.set_stream(tstream)
    stream = tstream.cuda_stream
    assert stream

    def timed(fn):
        fn()                                        # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(np.min(ms))

    rec = dict(batch=B, N=N, grid=[len(un), len(ut)], reps=a.reps, rows=[])
    for integ in ("euler", "rk4"):
        evals = (1 if integ == "euler" else 4) * N
        for name, fn in (("cost_landscape (NULL surface)", lambda: s.cost_landscape_device(lio, integrator=integ, stream=stream)),
                         ("rollout_cost M = 147", lambda: s.rollout_cost_device(rio, G, integrator=integ, stream=stream))):
            med, mn = timed(fn)
            row = dict(kernel=name, integrator=integ, ms_median=med, ms_min=mn, rollouts_per_s=B * G / (med * 1e-3),
                       stage_evals_per_s=B * G * N / (med * 1e-3), f_evals_per_s=B * G * evals / (med * 1e-3))
            rec["rows"].append(row)
            print(f"{name:32s} {integ:5s}  {med:8.3f} ms (min {mn:.3f})  {row['rollouts_per_s']:.3e} rollouts/s  "
                  f"{row['stage_evals_per_s']:.3e} stages/s  {row['f_evals_per_s']:.3e} f/s")
        # the two kernels agree bit for bit on the minimum
        torch.cuda.synchronize()
        same = bool(torch.equal(d_cost.min(1).values, d_cmin))
        print(f"  landscape cost_min == min of rollout_cost's surface: {same}")
        rec[f"bit_identical_{integ}"] = same
    s.close()
    if not a.no_cpu:
        import rollout_ref as R
        from oracle.oracle import Oracle
        orc = Oracle(NAMES, twin=True)
        nl = 64
        cand = R.landscape_candidates(tail[:nl], un, ut)
        for integ in ("euler", "rk4"):
            R.rollout_cost(orc, x0[:nl], cand[:, :4], sid[:nl], yref[:nl], yref[:nl, N - 1, :4], integrator=integ)
            t0 = time.perf_counter()
            R.rollout_cost(orc, x0[:nl], cand, sid[:nl], yref[:nl], yref[:nl, N - 1, :4], integrator=integ)
            dt = time.perf_counter() - t0
            row = dict(kernel="numpy restatement, 64 lanes", integrator=integ, ms_median=dt * 1e3,
                       rollouts_per_s=nl * G / dt, stage_evals_per_s=nl * G * N / dt,
                       threads=os.environ.get("OMP_NUM_THREADS", "all"))
            rec["rows"].append(row)
            print(f"{'numpy restatement, 64 lanes':32s} {integ:5s}  {dt * 1e3:8.3f} ms  {row['rollouts_per_s']:.3e} rollouts/s  "
                  f"{row['stage_evals_per_s']:.3e} stages/s  (OMP_NUM_THREADS={row['threads']})")
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
