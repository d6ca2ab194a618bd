"""Oracle study (CPU): why does a status-0 QP with active STATE bounds miss its exact solution?

The literal restatement's QP (oracle/qsp_oracle.c) is run in double, long double and __float128
(Oracle.qp / Oracle.qp_ext) on the manufactured QPs of tests/manufactured_qp.py, whose exact
primal-dual solutions are known by construction.  If the extended evaluation reaches the exact
solution, the formulas are right and the double answer is the rounding of the recursion; if it is
wrong too, a formula is.  Then the double error is measured against the multiplier range, the bound
offsets and the stop tolerance.  Per row, over the lanes that met the stop test (status 0):
  ok        their number, of 64
  du, lam   max |du - du*|, max |lam - lam*|
  stat_u    the u-stationarity residual of the returned du, pi, lam
  sig       the largest barrier weight lam / t at exit (t from the returned point)
  floor     the dual-accuracy floor of tests/test_oracle.py::test_qp_kkt, N sig eps max|lo, hi|
  model     eps sig^2: the rounding of a recursion that cancels a weight sig twice
Usage: python tests/tools/manufactured_qp_study.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import manufactured_qp as M  # noqa: E402
from oracle.oracle import Oracle, make_opts  # noqa: E402

EPS = np.finfo(float).eps
NB = 64


def row(orc, q, op, prec, label):
    a = M.qp_args(q)
    r = orc.qp(op, *a) if prec == "double" else orc.qp_ext(op, *a, precision=prec)
    m = r["qp_status"] == 0
    N = op.N
    if not m.any():
        print(f"{label:34s} {prec:6s} ok  0")
        return
    res = M.kkt_residuals(q, r["dx"], r["du"], r["pi"], r["lam"])
    v = np.concatenate([r["dx"][:, :N, 3:4], r["du"]], 2)
    t = np.stack([v - q["lo"], q["hi"] - v], 3).reshape(len(m), N, 6)
    t[:, 0, :2] = 1.0
    sig = (np.abs(r["lam"]) / np.maximum(np.abs(t), 1e-300))
    sig[:, 0, :2] = 0.0
    sig = sig.reshape(len(m), -1).max(1)
    off = np.maximum(np.abs(q["lo"]), np.abs(q["hi"])).reshape(len(m), -1).max(1)
    e = lambda k: np.abs(r[k][m] - q[k][m]).max()
    print(f"{label:34s} {prec:6s} ok {m.sum():2d} cap {np.sum(r['qp_status'] == 2):2d} du {e('du'):.1e} lam {e('lam'):.1e} "
          f"stat_u {res['stat_u'][m].max():.1e} sig {sig[m].max():.1e} floor {(N * sig * EPS * off)[m].max():.1e} "
          f"model {min(EPS * sig[m].max() ** 2, 9.9e99):.1e} iters {int(np.median(r['iters']))}", flush=True)


def main():
    orc = Oracle()
    print("# 1. precision: double / long double / __float128, generic scaling, mu_stop 1e-10")
    for fam in ("F0", "Fu", "Fs", "Fall"):
        for N in (3, 20, 50):
            q = M.make_batch(fam, N, NB, M.SEEDS.get(N, 1))
            op = make_opts(N=N, qp_iters=50, stage0_s_bound=0)
            for prec in ("double", "long", "quad"):
                row(orc, q, op, prec, f"{fam} N={N}")
    print("# 2. double, Fs, N = 20: the multiplier range")
    N = 20
    op = make_opts(N=N, qp_iters=50, stage0_s_bound=0)
    for lr in ((1e-4, 1e-3), (1e-3, 1e-2), (1e-2, 1e-1), (1e-1, 1.0), (1.0, 10.0)):
        row(orc, M.make_batch("Fs", N, NB, M.SEEDS.get(N, 1), lam_range=lr), op, "double", f"lam in [{lr[0]:g}, {lr[1]:g}]")
    print("# 3. double, Fs, N = 20, lam in [1e-3, 1e-2]: the bound offsets (dx*, du* and the widths scaled by c)")
    for c in (0.01, 0.1, 1.0, 10.0, 100.0):
        q = M.make_batch("Fs", N, NB, M.SEEDS.get(N, 1), lam_range=M.SMALL_LAM, sc_z=c, width=c * np.asarray(M.GENERIC["width"]))
        row(orc, q, op, "double", f"c = {c:g}")
    print("# 3b. double, Fs, N = 20, lam in [1e-2, 1e-1]: the scale of B (the OCP's is O(Ts))")
    for sc_B in (0.005, 0.05, 0.5, 5.0):
        row(orc, M.make_batch("Fs", N, NB, M.SEEDS.get(N, 1), lam_range=(1e-2, 1e-1), sc_B=sc_B), op, "double", f"sc_B = {sc_B:g}")
    print("# 4. double, Fs, N = 20, generic: the stop tolerances (mu_stop = res_stop = qp_tol_stat = qp_tol_eq)")
    q = M.make_batch("Fs", N, NB, M.SEEDS.get(N, 1))
    for tol in (1e-4, 1e-6, 1e-8, 1e-10):
        opt = make_opts(N=N, qp_iters=50, stage0_s_bound=0, mu_stop=tol, res_stop=tol, qp_tol_stat=tol, qp_tol_eq=tol)
        row(orc, q, opt, "double", f"tol = {tol:g}")
    print("# 5. quad, Fs, N = 20, generic: the same tolerances (the truncation of the stop test alone)")
    for tol in (1e-6, 1e-8, 1e-10):
        opt = make_opts(N=N, qp_iters=50, stage0_s_bound=0, mu_stop=tol, res_stop=tol, qp_tol_stat=tol, qp_tol_eq=tol)
        row(orc, q, opt, "quad", f"tol = {tol:g}")


if __name__ == "__main__":
    main()
