"""Bit patterns of every entry of the evaluators beside the solve path, for an A/B of two builds of the library
(developer tool, needs the GPU): qsp_eval_kkt, qsp_eval_kkt_device, qsp_qp_residuals, qsp_eval_sens,
qsp_eval_sens_device, qsp_get_sens and qsp_qp_sens on fixed seeded inputs.

  QSP_LIB_PATH=variants/parent.so python scripts/point_eval_ab.py --out parent.npz
  python scripts/point_eval_ab.py --out new.npz
  python scripts/point_eval_ab.py --compare parent.npz new.npz

Shapes: N in 1, 2, 20, 64, 127 (N = 1: the x_N row and both PI clamps fall on stage 0; N + 1 = 65: a lane spans
two waves of the KKT fold, 3 lanes per workgroup; N = 127: 2 lanes per workgroup, no tail) times B in 1, 7, 257
(7: no multiple of the lanes per workgroup; 257: one past a 256-thread block of the linearisation and one past
four 64-lane walk blocks), each on a handle with stage0_s_bound 0 and 1.  Options: LAM given, implied and (the
sensitivities) neither; x0 given and not; a shape_id override through the device entries; K and dU asked for and
not.  Every host call is made twice, once with a NaN in U (du, B) of lane B // 2 and once without: the run itself
checks that the bad lane's outputs are NaN and that every other lane has the same bits in both calls, and exits
with status 1 if not.  The inputs come from numpy alone, so two builds see the same numbers."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NS, BS = (1, 2, 20, 64, 127), (1, 7, 257)
NAMES = ("santal", "balea", "montana", "pulirapid")
SENS_ALL = ("K0", "K", "dU", "P0", "flag")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def point(s, seed):
    """A seeded point of the handle's (B, N) that needs no library call."""
    B, N = s.B, s.N
    rng = np.random.default_rng(seed)
    lh, uh = np.asarray(s._lh), np.asarray(s._uh)
    x0 = np.stack([rng.uniform(-0.01, 0.03, B), rng.uniform(-0.02, 0.01, B), rng.uniform(-0.15, 0.15, B),
                   rng.uniform(0.9 * lh[0] + 0.1 * uh[0], 0.1 * lh[0] + 0.9 * uh[0], B)], 1)
    X = x0[:, None] + np.cumsum(1e-3 * rng.uniform(-1, 1, (B, N + 1, 4)), 1)
    X[:, :, 3] = np.clip(X[:, :, 3], lh[0] - 1e-3, uh[0] + 1e-3)          # s on both sides of its bounds
    U = rng.uniform(lh[1:], uh[1:], (B, N, 2))
    PI = rng.uniform(-1.0, 1.0, (B, N, 4))
    LAM = np.where(rng.uniform(0, 1, (B, N, 6)) < 0.35, rng.uniform(0.0, 1.0, (B, N, 6)), 0.0)
    yref = 1e-2 * rng.uniform(-1, 1, (B, N, 6))
    yref_e = 1e-2 * rng.uniform(-1, 1, (B, 4))
    return dict(x0=x0, xa=x0 + 1e-4, X=X, U=U, PI=PI, LAM=LAM, yref=yref, yref_e=yref_e)


def qp_data(nb, N, seed):
    """Caller-QP arrays: A with the pusher-slider structure (qsp_qp_sens needs it), everything else of order one."""
    rng = np.random.default_rng(seed)
    A = np.tile(np.eye(4).reshape(16), (nb, N, 1))
    A[:, :, [2, 3, 6, 7, 11, 15]] += 0.1 * rng.uniform(-1, 1, (nb, N, 6))
    q = dict(A=A, B=0.1 * rng.uniform(-1, 1, (nb, N, 8)), b=1e-2 * rng.uniform(-1, 1, (nb, N, 4)),
             H=rng.uniform(0.5, 2.0, (nb, 6 * N + 4)), g=rng.uniform(-1, 1, (nb, 6 * N + 4)),
             lo=-rng.uniform(0.1, 1.0, (nb, N, 3)), dx0=1e-2 * rng.uniform(-1, 1, (nb, 4)),
             dx=rng.uniform(-1, 1, (nb, N + 1, 4)), du=rng.uniform(-1, 1, (nb, N, 2)), pi=rng.uniform(-1, 1, (nb, N, 4)),
             lam=rng.uniform(0, 1, (nb, N, 6)))
    q["hi"] = q["lo"] + rng.uniform(0.5, 2.0, (nb, N, 3))
    return q


class Run:
    def __init__(self):
        self.out, self.fails, self.pairs = {}, [], 0

    def put(self, key, arrays):
        for name, a in arrays.items():
            self.out[key + "/" + name] = np.ascontiguousarray(a)

    def pair(self, key, call, bad_lane, B):
        """call(bad) twice; the bad lane is NaN, the others keep their bits."""
        clean, bad = call(False), call(True)
        self.put(key + "/clean", clean)
        self.put(key + "/bad", bad)
        good = np.setdiff1d(np.arange(B), [bad_lane])
        self.pairs += 1
        for name in clean:
            if name == "flag":
                ok = bad[name][bad_lane] == 1 and not bad[name][good].any() and not clean[name].any()
            else:
                ok = np.all(np.isnan(bad[name][bad_lane])) and np.all(np.isfinite(clean[name]))
            if not (ok and np.array_equal(bits(bad[name][good]), bits(clean[name][good]))):
                self.fails.append(key + "/" + name)


def run_case(R, N, B, s0):
    import torch
    from uclv_qs_pushing_matlab_amd import _lib
    from uclv_qs_pushing_matlab_amd.objects import make_shape
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    key0 = "N%d_B%d_s%d" % (N, B, s0)
    sid = np.arange(B) % 4
    sid2 = ((np.arange(B) * 7 // 3) % 4).astype(np.int32)          # the override of the device entries
    s = OcpSolver(N=N, batch=B, sqp_iters=2, stage0_s_bound=bool(s0))
    s.set_shapes([make_shape(n) for n in NAMES], shape_id=sid)
    d = point(s, 1000 * N + B)
    bl = B // 2
    Ubad = d["U"].copy()
    Ubad[bl, N // 2, 1] = np.nan
    U = lambda bad: Ubad if bad else d["U"]
    s.set("cost_y_ref", d["yref"])
    s.set("cost_y_ref_e", d["yref_e"])
    dev = torch.device("cuda", 0)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    # --- KKT residuals of the point
    for lam in ("given", "implied"):
        for x0 in (True, False):
            def call(bad):
                r = s.eval_kkt(d["X"], U(bad), d["PI"], d["LAM"] if lam == "given" else "implied", x0=d["xa"] if x0 else None,
                               yref=d["yref"], yref_e=d["yref_e"], parts=True, stages=True)
                return dict(zip(("res", "parts", "stage_res"), r))
            R.pair("%s/kkt/lam=%s/x0=%d" % (key0, lam, x0), call, bl, B)
    ins = dict(x0=t(d["xa"]), X=t(d["X"]), U=t(d["U"]), PI=t(d["PI"]), LAM=t(d["LAM"]), yref=t(d["yref"]),
               yref_e=t(d["yref_e"]), shape_id=t(sid2))
    outs = dict(res=torch.zeros((B, 4), dtype=torch.float64, device=dev),
                parts=torch.zeros((B, 7), dtype=torch.float64, device=dev),
                stage_res=torch.zeros((B, N + 1, 4), dtype=torch.float64, device=dev))
    io = _lib.KktIO()
    for k, v in list(ins.items()) + list(outs.items()):
        setattr(io, k, v.data_ptr())
    torch.cuda.synchronize()
    s.eval_kkt_device(io)
    s.synchronize()
    R.put(key0 + "/kkt_device/shape_id", {k: v.cpu().numpy() for k, v in outs.items()})
    # --- residuals of a QP point
    q = qp_data(B, N, 7000 * N + B)
    dubad = q["du"].copy()
    dubad[bl, N // 2, 0] = np.nan

    def call(bad):
        return s.qp_residuals(*[q[k] for k in ("A", "B", "b", "H", "g", "lo", "hi", "dx0", "dx")], dubad if bad else q["du"],
                              q["pi"], q["lam"])
    R.pair(key0 + "/qp_residuals", call, bl, B)
    # --- sensitivities of the point
    for mult, kw in (("given", dict(PI=d["PI"], LAM=d["LAM"])), ("implied", dict(PI=d["PI"])), ("none", dict())):
        for x0 in (True, False):
            def call(bad):
                return s.eval_sens(d["X"], U(bad), x0=d["xa"] if x0 else None, want=SENS_ALL, **kw)
            key = "%s/sens/lam=%s/x0=%d" % (key0, mult, x0)
            R.pair(key, call, bl, B)
            R.put(key + "/K0_only", s.eval_sens(d["X"], d["U"], x0=d["xa"] if x0 else None, **kw))
        R.put("%s/sens/lam=%s/s0_bound=%d" % (key0, mult, 1 - s0),
              s.eval_sens(d["X"], d["U"], want=SENS_ALL, s0_bound=bool(1 - s0), **kw))
    shapes = dict(K0=(B, 2, 4), K=(B, N, 2, 4), dU=(B, N, 2, 4), P0=(B, 10))
    for names in (SENS_ALL, ("K0", "flag")):
        souts = {k: torch.zeros(shapes[k], dtype=torch.float64, device=dev) for k in names if k != "flag"}
        souts["flag"] = torch.zeros((B,), dtype=torch.int32, device=dev)
        io = _lib.SensIO()
        for k in ("x0", "X", "U", "PI", "yref", "shape_id"):          # implied multipliers, the references given
            setattr(io, k, ins[k].data_ptr())
        for k, v in souts.items():
            setattr(io, k, v.data_ptr())
        torch.cuda.synchronize()
        s.eval_sens_device(io)
        s.synchronize()
        R.put("%s/sens_device/shape_id/%s" % (key0, "+".join(names)), {k: v.cpu().numpy() for k, v in souts.items()})
    # --- the walk on caller-given QP data
    Bbad = q["B"].copy()
    Bbad[bl, N // 2, 3] = np.nan
    R.pair(key0 + "/qp_sens", lambda bad: s.qp_sens(q["A"], Bbad if bad else q["B"], q["H"], want=SENS_ALL), bl, B)
    R.put(key0 + "/qp_sens/K0_only", s.qp_sens(q["A"], q["B"], q["H"]))
    # --- the last solve's iterate
    s.set("constr_x0", d["x0"])
    s.set("init_x", np.repeat(d["x0"][:, None], N + 1, 1))
    s.set("init_u", np.zeros((B, N, 2)))
    s.solve()
    R.put(key0 + "/get_sens", s.get_sens(want=SENS_ALL))
    s.close()


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    print("%s: %d arrays; %s: %d arrays; names %s" % (pa, len(a.files), pb, len(b.files),
                                                     "SAME" if set(a.files) == set(b.files) else "DIFF"))
    bad = sorted(set(a.files) ^ set(b.files))
    groups = {}
    for k in sorted(set(a.files) & set(b.files)):
        same = a[k].shape == b[k].shape and np.array_equal(bits(a[k]), bits(b[k]))
        g = groups.setdefault(k.split("/")[0], [0, 0, 0])
        g[0] += 1
        g[1] += same
        g[2] += a[k].size
        if not same:
            bad.append(k)
    for g, (n, ok, words) in groups.items():
        print("%-14s %4d arrays, %9d words: %s" % (g, n, words, "bit-identical" if n == ok else "%d DIFFER" % (n - ok)))
    for k in bad:
        print("DIFF  " + k)
    print("%d of %d arrays differ" % (len(bad), len(set(a.files) | set(b.files))))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, default=None)
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    R = Run()
    for N in NS:
        for B in BS:
            for s0 in (0, 1):
                run_case(R, N, B, s0)
    from uclv_qs_pushing_matlab_amd import LIB_PATH
    print("%s: %d arrays from %d handles; %d bad-lane pairs, %d arrays beside a bad lane changed or a bad lane not NaN"
          % (LIB_PATH, len(R.out), len(NS) * len(BS) * 2, R.pairs, len(R.fails)))
    for k in R.fails:
        print("FAIL  " + k)
    if a.out:
        np.savez(a.out, **R.out)
    sys.exit(1 if R.fails else 0)


if __name__ == "__main__":
    main()
