"""Rate of the batched closed loop with a plant model of its own and with on-device metrics (developer tool,
needs the GPU).

main.m's scenario (Hp = 10, sqp + merit backtracking, max_iter 30, QP cap 50, 201 steps of Ts = 0.05, the
straight-line reference, no noise, no delay), four shapes mixed per lane, x0 from the config-2 law, at B = 65 536:
  (a) qsp_closed_loop_ex of a library built from the parent commit (--parent-lib; without it the row is left out);
  (b) qsp_closed_loop_ex of this tree with no plant installed;
  (c) the same with per-lane mu_sp / c_ellipse (qsp_set_plant_params: +-20 % around each lane's shape);
  (d) qsp_closed_loop_metrics with the same plant;
  (e) qsp_closed_loop_metrics, no plant, sim_noise from a host table (n_steps x B x 4 doubles: 421 MB at this size),
      here the table that qsp_gen_sim_noise writes; the time numpy takes to draw the equivalent table on the host
      (helper.py's default path) is reported on its own;
  (f) the same run with the generator installed (qsp_set_sim_noise) and noise = NULL: the same noise values drawn
      in closed_loop_pre_kernel, no table anywhere.
Both libraries are driven through the C ABI alone (ctypes), so that the parent's older ABI loads, and each runs in
a process of its own, started afresh for every repetition (with both handles alive in one process the two
libraries did not time alike although their kernels are the same code: profiles/plant_model/README.md).  The legs
are interleaved, repetition by repetition: (a), then (b) to (f) on one handle, after a warm-up of three steps.
Per row: the loop's own HIP-event time (qsp_get_time_tot: all kernels of the 201 steps, no copy) as median,
minimum and maximum, lane-steps/s from the median, and the median wall time of the call, which adds the host
copies (about 0.7 GB of trajectories for (a)-(c), 5 MB of metrics for (d) and (f), the 421 MB table for (e)).  (b)
against (a) is the regression check: (b)'s median must lie within (a)'s own minimum-to-maximum spread.  (f) against
(e): the same noise, so the same solver work (x_end and status equal); (f)'s median within or below (e)'s spread.

  python scripts/closed_loop_mc_rate.py [--batch 65536] [--steps 201] [--reps 7] [--parent-lib FILE] [--legs bcdef]
                                        [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ("santal", "balea", "montana", "pulirapid")
USED = ("qsp_default_options", "qsp_create", "qsp_destroy", "qsp_set_shapes", "qsp_set_shape_ids",
        "qsp_set_reference_trajectory", "qsp_closed_loop_ex", "qsp_get_time_tot", "qsp_last_error")
NEW = ("qsp_set_plant_params", "qsp_clear_plant", "qsp_closed_loop_metrics", "qsp_default_sim_noise",
       "qsp_set_sim_noise", "qsp_clear_sim_noise", "qsp_gen_sim_noise")
METRICS = ("sum_exy2", "max_exy2", "sum_eth2", "end_exy2", "sum_u2", "n_failed", "n_st", "n_sl", "n_sr", "n_s_out")


def config2_x0(nb, seed):   # BASELINE config 2 initial-state law (main.m:53-56 ranges)
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-0.0065, 0.0260, nb), rng.uniform(-0.0197, 0.0124, nb),
                     np.deg2rad(rng.uniform(-8.05, 9.30, nb)), rng.uniform(-0.0382, 0.0011, nb)], 1)


def straight_traj(T_end=10.0, Ts=0.05, v=0.01):
    t = np.arange(0.0, T_end + 1e-9, Ts)
    traj = np.zeros((len(t), 6))
    traj[:, 0] = v * t
    return traj


class Handle:
    """One solver handle of one library, through the C ABI."""

    def __init__(self, path, B, shapes, sid, traj, new_abi):
        from uclv_qs_pushing_matlab_amd import _lib
        self.L = C.CDLL(path)
        for name in USED + (NEW if new_abi else ()):
            fn = getattr(self.L, name)
            fn.argtypes = _lib._SIGS[name]
            fn.restype = None if name in _lib._VOID else C.c_char_p if name == "qsp_last_error" else C.c_int
        o = _lib.Options()
        self.L.qsp_default_options(C.byref(o))
        o.N, o.batch, o.sqp_iters, o.qp_iters, o.nlp_mode = 10, B, 30, 50, 1
        self.h = C.c_void_p()
        self.ok(self.L.qsp_create(C.byref(o), C.byref(self.h)))
        arr = (_lib.Shape * len(shapes))(*shapes)
        self.ok(self.L.qsp_set_shapes(self.h, arr, len(shapes)))
        self.ok(self.L.qsp_set_shape_ids(self.h, sid.ctypes.data))
        self.ok(self.L.qsp_set_reference_trajectory(self.h, traj.ctypes.data, len(traj)))

    def ok(self, rc):
        if rc != 0:
            raise RuntimeError(f"C ABI call failed ({rc}): {self.L.qsp_last_error().decode()}")

    def time_tot(self):
        ms = C.c_double()
        self.ok(self.L.qsp_get_time_tot(self.h, C.byref(ms)))
        return ms.value

    def close(self):
        self.L.qsp_destroy(self.h)


def worker(a):
    """One library in this process: its handle, a short warm-up, then the rows asked for, one line each."""
    import hashlib
    import torch  # noqa: F401  (one HIP runtime per process: uclv_qs_pushing_matlab_amd/_lib.py)
    from uclv_qs_pushing_matlab_amd import _lib
    from uclv_qs_pushing_matlab_amd.objects import make_shape
    B, T = a.batch, a.steps
    shapes = [make_shape(n) for n in NAMES]
    sid = (np.arange(B) % 4).astype(np.int32)
    x0 = np.ascontiguousarray(config2_x0(B, 0))
    idx = np.ones(B, np.int32)
    rng = np.random.default_rng(2)
    mu = np.array([s.mu_sp for s in shapes])[sid] * rng.uniform(0.8, 1.2, B)
    ce = np.array([s.c_ellipse for s in shapes])[sid] * rng.uniform(0.8, 1.2, B)
    hd = Handle(a.parent_lib or _lib.LIB_PATH, B, shapes, sid, straight_traj(), not a.parent_lib)
    X, U, S = np.zeros((B, T + 1, 4)), np.zeros((B, T, 2)), np.zeros((B, T), np.int32)
    met, xe, st = np.zeros((B, 10)), np.zeros((B, 4)), np.zeros(B, np.int32)
    p = lambda v: v.ctypes.data  # noqa: E731

    def loop(n):
        hd.ok(hd.L.qsp_closed_loop_ex(hd.h, None, p(x0), p(idx), n, None, p(X), None, p(U), p(S)))

    def metrics(n, noise=None):
        hd.ok(hd.L.qsp_closed_loop_metrics(hd.h, None, p(x0), p(idx), n, None if noise is None else p(noise), p(met),
                                           p(xe), p(st)))

    def generator(on):
        if on:
            g = _lib.SimNoise()
            hd.L.qsp_default_sim_noise(C.byref(g))
            g.seed = 20250303
            hd.ok(hd.L.qsp_set_sim_noise(hd.h, C.byref(g)))
        else:
            hd.ok(hd.L.qsp_clear_sim_noise(hd.h))

    loop(3)                                        # warm-up: code objects, allocations, host pages
    if set("def") & set(a.rows):
        metrics(3)
    table, e_end = None, None
    if "e" in a.rows:                              # the table of (f)'s generator, and numpy's draw of such a table
        table = np.zeros((T, B, 4))
        generator(True)
        hd.ok(hd.L.qsp_gen_sim_noise(hd.h, T, p(table)))
        generator(False)
        metrics(3, table)                          # warm-up of the table's device buffer
        t0 = time.perf_counter()
        np.random.default_rng(0).standard_normal((T, B, 4)) * np.array([1e-5, 1e-5, 1e-3, 1e-4])
        draw = (time.perf_counter() - t0) * 1e3
    X[:], U[:], S[:] = 0.0, 0.0, 0
    for row in a.rows:
        if row in "ef":
            generator(row == "f")
            t0 = time.perf_counter()
            metrics(T, table if row == "e" else None)
            wall = (time.perf_counter() - t0) * 1e3
            ms = hd.time_tot()
            generator(False)
            h = hashlib.sha256(xe.tobytes() + st.tobytes() + met.tobytes()).hexdigest()[:16]
            note = f"sha {h} " + (f"numpy_draw_ms {draw:.1f}" if row == "e" else
                                  f"is_e {int(e_end is not None and h == e_end)}")
            e_end = h if row == "e" else e_end
            print(f"ROW {row} {ms:.3f} {wall:.3f} {note}", flush=True)
            continue
        if row in "cd":
            hd.ok(hd.L.qsp_set_plant_params(hd.h, p(mu), p(ce)))
        t0 = time.perf_counter()
        metrics(T) if row == "d" else loop(T)
        wall = (time.perf_counter() - t0) * 1e3
        ms = hd.time_tot()
        if row in "cd":
            hd.ok(hd.L.qsp_clear_plant(hd.h))
        if row == "d":   # after (c) in the same process: X, S still hold (c)'s run
            note = (f"x_end_is_c {int(np.array_equal(xe, X[:, T]))} status_is_c {int(np.array_equal(st, S[:, T - 1]))} "
                    + " ".join(f"{v:.3e}" for v in np.median(met, 0)))
        else:
            h = hashlib.sha256(X.tobytes() + U.tobytes() + S.tobytes()).hexdigest()[:16]
            note = f"sha {h} mean_x_end {float(np.abs(X[:, T, :2]).mean()):.6e}"
        print(f"ROW {row} {ms:.3f} {wall:.3f} {note}", flush=True)
    hd.close()


LABEL = {"a": "(a) closed_loop_ex, parent commit", "b": "(b) closed_loop_ex, no plant installed",
         "c": "(c) closed_loop_ex, per-lane mu_sp / c_ellipse", "d": "(d) closed_loop_metrics, the same plant",
         "e": "(e) closed_loop_metrics, noise from a host table", "f": "(f) closed_loop_metrics, noise drawn on device"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=201)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-lib", default=None, help="libqsp_nmpc.so built from the parent commit, for row (a)")
    ap.add_argument("--legs", default="bcdef", help="rows of this tree to run, e.g. bef (b is always needed with --parent-lib)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default=None, help=argparse.SUPPRESS)   # worker: the rows of one library
    a = ap.parse_args()
    if a.rows:
        return worker(a)
    import subprocess
    B, T = a.batch, a.steps
    legs = ([("a", ["--parent-lib", a.parent_lib])] if a.parent_lib else []) + [(a.legs, [])]
    ms, wall, notes = {}, {}, {}
    for _ in range(a.reps):                        # interleaved: one repetition of every row in turn
        for rows, extra in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--batch", str(B), "--steps", str(T), "--rows", rows] + extra
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:                  # nothing more is started on the GPU after a failure
                sys.exit(f"worker {rows} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            for ln in r.stdout.splitlines():
                if ln.startswith("ROW "):
                    print(ln, file=sys.stderr, flush=True)
                    _, row, m, w, note = ln.split(" ", 4)
                    ms.setdefault(row, []).append(float(m))
                    wall.setdefault(row, []).append(float(w))
                    notes.setdefault(row, []).append(note)
    lines = [f"closed-loop Monte-Carlo rate: B = {B}, {T} steps, N = 10, merit SQP (max_iter 30, QP cap 50), four shapes; "
             f"{a.reps} interleaved repetitions, each library in a process of its own; device time = the loop's HIP "
             "events, wall = the whole call"]
    for k in sorted(ms):
        med, lo, hi = float(np.median(ms[k])), float(np.min(ms[k])), float(np.max(ms[k]))
        lines.append(f"{LABEL[k]:50s} {med:9.1f} ms (min {lo:.1f}, max {hi:.1f})  {B * T / (med * 1e-3):.3e} lane-steps/s  "
                     f"wall {float(np.median(wall[k])):9.1f} ms")
    if "a" in ms:
        inside = float(np.min(ms["a"])) <= float(np.median(ms["b"])) <= float(np.max(ms["a"]))
        same = len(set(n.split()[1] for n in notes["a"] + notes["b"])) == 1
        lines.append(f"(b) median within (a)'s min..max: {inside}; (a) and (b) bit-identical in X, U, status "
                     f"(sha-256 of every repetition): {same}")
    if "c" in notes:
        lines.append(f"(c): {notes['c'][-1]}; (b): {notes['b'][-1]}")
    if "d" in notes:
        d = notes["d"][-1].split()
        lines.append(f"(d) x_end == (c) X[:, -1]: {bool(int(d[1]))}; status: {bool(int(d[3]))}; medians over lanes of the "
                     f"ten metrics ({', '.join(METRICS)}): {' '.join(d[4:])}")
    if "e" in ms and "f" in ms:
        same = all(n.split()[3] == "1" for n in notes["f"])
        fm = float(np.median(ms["f"]))
        lines.append(f"(f) metrics, x_end and status bit-identical to (e)'s on every repetition: {same}; (f) median within or "
                     f"below (e)'s min..max: {fm <= float(np.max(ms['e']))}; numpy's draw of a {T} x {B} x 4 table on the "
                     f"host (not part of (e)'s times): median {float(np.median([float(n.split()[3]) for n in notes['e']])):.1f} ms")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
