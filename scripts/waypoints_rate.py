"""Rate of per-lane waypoint reference tables generated on the device (developer tool, needs the GPU).

Workload: B = 65 536 lanes, each main.m:141-148's three-segment path (0, 0) -> (0.12, 0) -> (0.12, 0.06) ->
(0.12, 0.12) scaled by a factor of its own drawn from [0.5, 1.5], at 0.01 m/s and Ts = 0.05: 241 to 721 samples per
lane, the table B x T x 6 doubles with T the longest lane's.
  (a) qsp_gen_waypoints: the host prepares O(B K) numbers, waypoints_kernel writes the table on the device;
  (b) the path a user had before it: TrajectoryGenerator.waypoints_gen (the numpy mirror) lane by lane into a
      B x T x 6 host array, the last row repeated up to T, then qsp_set_reference_trajectories.  Taken on --np-lanes
      lanes (1 024: a handle of that batch, the first lanes of the same draw, padded to the same T) and scaled by
      B / np-lanes, since it is one Python loop over the lanes and a copy in proportion; the record says so.
Both are wall times of the whole call, which ends after a synchronise of the handle's stream; --reps repetitions
each, after one warm-up call, as median and range.  The tables of the first np-lanes lanes are compared.

  python scripts/waypoints_rate.py [--batch 65536] [--np-lanes 1024] [--reps 5] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PATH = np.array([[0.0, 0.0], [0.12, 0.0], [0.12, 0.06], [0.12, 0.12]])   # main.m:141-148
VEL, TS = 0.01, 0.05


def mirror_table(wp, T):
    """(b)'s host side: the numpy mirror per lane, padded with the last row to T rows."""
    from uclv_qs_pushing_matlab_amd.trajectory import TrajectoryGenerator
    tab = np.zeros((len(wp), T, 6))
    for i in range(len(wp)):
        tg = TrajectoryGenerator(TS, VEL)
        tg.waypoints_, tg.waypoints_velocities = wp[i], [VEL]
        _, tr = tg.waypoints_gen()
        n = tr.shape[1]
        tab[i, :n, :4] = tr[:4].T
        tab[i, n:] = tab[i, n - 1]
    return tab


def stats(v):
    return f"median {np.median(v):9.1f} ms (min {np.min(v):.1f}, max {np.max(v):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--np-lanes", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from uclv_qs_pushing_matlab_amd.objects import make_shape
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    B, nb = a.batch, min(a.np_lanes, a.batch)
    wp = PATH[None] * np.random.default_rng(0).uniform(0.5, 1.5, B)[:, None, None]

    s = OcpSolver(N=10, batch=B)
    s.set_shapes([make_shape("santal")])
    T, T_lane = s.gen_waypoints(wp, VEL)                         # warm-up: code object, the table's allocation
    dev = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        s.gen_waypoints(wp, VEL)
        dev.append((time.perf_counter() - t0) * 1e3)
    s.close()

    # the first nb lanes of the table for the comparison, from a handle of nb lanes (T is the whole batch's)
    h = OcpSolver(N=10, batch=nb)
    h.set_shapes([make_shape("santal")])
    h.gen_waypoints(wp[:nb], VEL)
    got = h.get_reference_trajectories()
    got = np.concatenate([got, np.repeat(got[:, -1:], T - got.shape[1], axis=1)], axis=1)
    h.set_reference_trajectories(mirror_table(wp[:8], T).repeat(nb // 8 + 1, axis=0)[:nb])   # warm-up
    host, build = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        tab = mirror_table(wp[:nb], T)
        t1 = time.perf_counter()
        h.set_reference_trajectories(tab)
        host.append((time.perf_counter() - t0) * 1e3)
        build.append((t1 - t0) * 1e3)
    h.close()
    err = float(np.abs(got[:, :, :4] - tab[:, :, :4]).max())
    scale = B / nb
    size = B * T * 6 * 8
    lines = [f"waypoint reference tables: B = {B} lanes of main.m:141-148's three-segment path scaled by U[0.5, 1.5] per lane, "
             f"{VEL} m/s, Ts = {TS}: {int(T_lane.min())} to {T} samples per lane, table B x {T} x 6 doubles = "
             f"{size / 1e9:.2f} GB; wall time of the whole call after a synchronise, {a.reps} repetitions",
             f"(a) qsp_gen_waypoints, B = {B}:                        {stats(dev)}  "
             f"{B / (np.median(dev) * 1e-3):.3e} lanes/s, {size / (np.median(dev) * 1e-3) / 1e9:.1f} GB/s of table",
             f"(b) numpy mirror per lane + qsp_set_reference_trajectories, measured on {nb} lanes:  {stats(host)}, "
             f"of which the mirror's loop {stats(build)}",
             f"(b) scaled to B = {B} (x {scale:g}; not measured at that size):    median {np.median(host) * scale / 1e3:9.1f} s "
             f"(min {np.min(host) * scale / 1e3:.1f}, max {np.max(host) * scale / 1e3:.1f}); "
             f"(b) scaled / (a) = {np.median(host) * scale / np.median(dev):.0f}",
             f"largest |device - mirror| over x, y, yaw, s_ref of the first {nb} lanes, every sample: {err:.3e}"]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
