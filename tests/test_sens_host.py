"""CPU: csrc/qsp_sens.hpp itself, compiled for the host in a program of its own (tests/stubs/sens_main.cpp): the
sensitivity walk of qsp_qp_sens' kernel (sens_back_step, which calls the solver's ric_factor_step, and
sens_fwd_step) on manufactured QP data (tests/manufactured_qp.py, nb = 7, N = 3 and 20) with a barrier diagonal
in H (tests/sens_ref.py::barrier_H), against the dense KKT solve of tests/sens_ref.py, which uses no Riccati
recursion.  Built with the address and undefined-behaviour sanitizers; nothing is loaded into Python.

Two barrier patterns:
  mixed   zero on most sides, 1e2 .. 1e10 on a seeded tenth, both inputs of a stage pinned (1e10, 1e8), an s side
          pinned at stage 1 (1e10) and at stage N - 1 (1e6);
  inputs  the same draw with every s entry at zero.

Bound: |host - dense| <= BOUND * eps * |row| * cond, per output -- |row| the largest entry of the reference's
row (a gain's row of four; P0: the lane's largest entry), cond the 2-norm condition number numpy reports for
the lane's whole-horizon KKT matrix (up to 4e11 here).  The dense solve is only backward stable, hence a scale
of the eps * cond type; BOUND is eight times the worst ratio measured here on the CPU:
                     K0        K         dU        P0
    inputs  N = 3    0.187     0.187     0.544     0.0439
    inputs  N = 20   6.98e-9   3.30e-8   1.75e-7   2.89e-9
    mixed   N = 3    0.187     0.187     0.244     5.47
    mixed   N = 20   1.27e4    4.77e4    2.59e4    3.02e3
What the mixed figures at N = 20 say: with input bounds pinned alone the walk agrees with the dense solve to a few
eps relative (the ratios at N = 20 are small because every lane there has cond >= 3e8, which overstates the
dense solve's error), but an s side
pinned in mid-horizon by d >~ 1e7 costs the Riccati recursion digits -- relative error of K0 4e-6 at d = 4e7, 0.44
on the lane with d = 7e9 at stages 4 and 11 (the dense solve is the accurate one: eps * cond <= 4e-5).  That is
the double-precision limit of the recursion under state-bound barrier weights that DESIGN.md section 2 and
tests/test_manufactured_qp.py record for the QP solver itself (P = Q + S'K cancels the weight twice), here
through the same ric_factor_step.  The mixed bound at N = 20 therefore holds the walk only to that limit; the
inputs pattern holds it to rounding.
"""
import numpy as np
import pytest

import host_program
import manufactured_qp as mq
import sens_ref

# 8 x the worst measured ratio of each (pattern, N), rounded up
BOUND = {("inputs", 3): 4.4, ("inputs", 20): 1.4e-6, ("mixed", 3): 44.0, ("mixed", 20): 3.9e5}
NB, SEED = 7, 1


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return host_program.build("sens_main", tmp_path_factory.mktemp("sens") / "sens_main")


@pytest.mark.parametrize("N", [3, 20])
@pytest.mark.parametrize("pattern", ["inputs", "mixed"])
def test_sens_walk_on_the_host(exe, tmp_path, pattern, N):
    q = mq.make_batch("Fall", N, NB, SEED)
    H, pins = sens_ref.barrier_H(q, SEED, s_pins=(pattern == "mixed"))
    got = sens_ref.run_host_program(exe, tmp_path / "q.bin", q["A"], q["B"], H)
    ref = sens_ref.sens(q["A"], q["B"], H)
    assert not got["flag"].any()
    bound = BOUND[pattern, N]
    worst = {}
    for name in sens_ref.OUTPUTS:
        scale = sens_ref.row_scale(ref, name)
        worst[name] = float((np.abs(got[name] - ref[name]) / scale).max())
    print("%s N = %d: cond %.1e .. %.1e; worst |host - dense| / (eps |row| cond): %s"
          % (pattern, N, ref["cond"].min(), ref["cond"].max(), {k: "%.3g" % v for k, v in worst.items()}))
    for name in sens_ref.OUTPUTS:
        scale = sens_ref.row_scale(ref, name)
        assert np.all(np.abs(got[name] - ref[name]) <= bound * scale), (name, worst[name])
    # K0 is the first stage of K and of dU (Phi_0 = I), bit for bit
    assert np.array_equal(got["K0"], got["K"][:, 0]) and np.array_equal(got["K0"], got["dU"][:, 0])
    # A pinned input hardly moves: its row of K_k is the numerator B_k' lam over Hu + d (the stationarity of
    # du_k), so below numerator / d -- the numerator is of order one (below 100 here, asserted), and a barrier at a
    # wrong index leaves the row at order one, 1e6 .. 1e10 times too large.
    assert len(pins) >= 3
    for l, k, i, d in pins:
        rowmax = np.abs(got["K"][l, k, i]).max()
        numer = np.abs(ref["numer"][l, k, i]).max()
        tol = bound * sens_ref.row_scale(ref, "K")[l, k, i].max()
        assert rowmax <= numer / d + tol and rowmax * d < 100.0, (l, k, i, d, rowmax, numer)
