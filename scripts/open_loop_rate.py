"""Rate of the open-loop kernel and of its two trajectory store paths (developer tool, needs the GPU).

Times, with HIP events on device-resident data after a warm-up and outside any copy, qsp_open_loop_device at
B = 65 536, M = 1, T = 200, four shapes, clip on, no delay, no noise:
  (a) x_end only (no trajectory is stored);
  (b) all outputs, every thread storing its own rows (store_tile = 1);
  (c) all outputs, 8 steps per thread collected in LDS and written out coalesced (store_tile = 8), and the
      same with 4 steps (store_tile = 4);
  (d) qsp_rollout_cost_device, Euler, N = 20, M = 10: the same 200 Euler steps per lane, the yardstick for (a).
The same five rows follow for B / 64 lanes x M = 64 candidates (one lane per workgroup, its shape in LDS).
All rows of a table are interleaved, repetition by repetition; each row reports the median, the minimum and the
maximum of the repetitions, Euler steps per second and, for (b) and (c), the achieved GB/s of the bytes
written.  The outputs of (b) and (c) are compared bit for bit at this size.

  python scripts/open_loop_rate.py [--batch 65536] [--steps 200] [--reps 7] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ("santal", "balea", "montana", "pulirapid")


def config2_x0(nb, seed):   # BASELINE config 2 initial-state law (main.m:53-56 ranges)
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-0.0065, 0.0260, nb), rng.uniform(-0.0197, 0.0124, nb),
                     np.deg2rad(rng.uniform(-8.05, 9.30, nb)), rng.uniform(-0.0382, 0.0011, nb)], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = []
    for B, M in ((a.batch, 1), (max(a.batch // 64, 1), 64)):   # M = 64: one lane per workgroup, shape in LDS
        out += measure(a, B, M)
    print("\n".join(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(out) + "\n")


def measure(a, B, M):
    import torch
    from uclv_qs_pushing_matlab_amd import _lib
    from uclv_qs_pushing_matlab_amd.objects import make_shape
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    T = a.steps
    Nr, Mr = 20, M * (T // 20)                     # (d): Mr candidates of Nr steps = M T steps per lane
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    x0 = config2_x0(B, 21)
    sid = (np.arange(B) % 4).astype(np.int32)
    U = np.stack([rng.uniform(0.001, 0.03, (B, M)), rng.uniform(-0.05, 0.05, (B, M))], -1)

    s = OcpSolver(N=Nr, batch=B)
    s.set_shapes([make_shape(n) for n in NAMES], shape_id=sid)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    z = lambda *shape, dt=torch.float64: torch.zeros(*shape, dtype=dt, device=dev)
    d_x0, d_U = t(x0), t(U)

    def buffers():
        return dict(X=z(B, M, T + 1, 4), U_out=z(B, M, T, 2), S_p=z(B, M, T, 2), mode=z(B, M, T, dt=torch.int32),
                    mode_steps=z(B, M, 4, dt=torch.int32), x_end=z(B, M, 4))

    def io_of(buf, traj):
        io = _lib.OpenLoopIO()
        io.x0, io.U, io.x_end = d_x0.data_ptr(), d_U.data_ptr(), buf["x_end"].data_ptr()
        if traj:
            for k in ("X", "U_out", "S_p", "mode", "mode_steps"):
                setattr(io, k, buf[k].data_ptr())
        return io

    bufs = {k: buffers() for k in ("direct", "tile8", "tile4")}
    end_only = dict(x_end=z(B, M, 4))
    written = B * M * ((T + 1) * 32 + T * (16 + 16 + 4) + 16 + 32)       # bytes of all outputs
    # (d) the rollout yardstick
    d_Ur = t(np.repeat(np.repeat(U[:, :, None], Nr, 2), Mr // M, 1))
    d_yref, d_ye, d_cost = z(B, Nr, 6), z(B, 4), z(B, Mr)
    rio = _lib.RolloutIO()
    rio.x0, rio.U, rio.yref, rio.yref_e, rio.cost = (d_x0.data_ptr(), d_Ur.data_ptr(), d_yref.data_ptr(),
                                                     d_ye.data_ptr(), d_cost.data_ptr())
    # a stream of our own: the events and the launches must share it
    tstream = torch.cuda.Stream()
    torch.cuda.synchronize()
    torch.cuda.set_stream(tstream)
    stream = tstream.cuda_stream
    assert stream

    runs = {
        "(a) x_end only": lambda: s.open_loop_device(io_of(end_only, False), T, M, stream=stream),
        "(b) all outputs, direct stores": lambda: s.open_loop_device(io_of(bufs["direct"], True), T, M, store_tile=1, stream=stream),
        "(c) all outputs, LDS tile of 8 steps": lambda: s.open_loop_device(io_of(bufs["tile8"], True), T, M, store_tile=8, stream=stream),
        "(c4) all outputs, LDS tile of 4 steps": lambda: s.open_loop_device(io_of(bufs["tile4"], True), T, M, store_tile=4, stream=stream),
        "(d) rollout_cost Euler N = 20, M = %d" % Mr: lambda: s.rollout_cost_device(rio, Mr, integrator="euler", stream=stream),
    }
    ms = {k: [] for k in runs}
    for fn in runs.values():                       # warm-up of every shape the timed window uses
        fn()
    torch.cuda.synchronize()
    for _ in range(a.reps):                        # interleaved: one repetition of every run in turn
        for k, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    torch.cuda.synchronize()
    lines = [f"open-loop rate: B = {B}, M = {M}, T = {T}, four shapes, clip on; {a.reps} interleaved repetitions; "
             f"bytes written by (b), (c): {written / 1e6:.1f} MB"]
    for k, v in ms.items():
        med, lo, hi = float(np.median(v)), float(np.min(v)), float(np.max(v))
        row = f"{k:40s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})  {B * M * T / (med * 1e-3):.3e} Euler steps/s"
        if "all outputs" in k:
            row += f"  {written / (med * 1e-3) / 1e9:8.1f} GB/s written"
        lines.append(row)
    same = all(torch.equal(bufs["direct"][k], bufs[o][k]) for o in ("tile8", "tile4") for k in bufs["direct"])
    same_end = bool(torch.equal(end_only["x_end"], bufs["direct"]["x_end"]))
    lines.append(f"outputs of (b), (c), (c4) bit-identical: {same}; x_end of (a) == x_end of (b): {same_end}")
    lines.append(f"store_tile = 0 runs {'(b)' if M >= 64 else '(c4)'} at this M (ol_default_tile, csrc/qsp_openloop.hip)")
    s.close()
    torch.cuda.set_stream(torch.cuda.default_stream())
    return lines


if __name__ == "__main__":
    main()
