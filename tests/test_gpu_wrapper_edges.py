"""GPU: the two device paths around the solve that no other GPU test compares with the twin.

Staging edges: stage_yref_kernel in the delay prefix of the reference table (index_time + k <= delay_cols),
at its end clamp, and on a per-lane table.  QP status codes: qsp_qp_solve's qp_status 2 (cap) and 3
(infeasible stage-0 s), which test_gpu_twin.py's QPs never reach.  Both sides call one function for each
(stage_yref, qp_exit_status, qp_level_status: csrc/qsp_ipm.hpp), so the expected result is equality of every
bit; the inputs are those of tests/twin_bits_cases.py, whose twin outputs tests/golden/twin_bits.npz pins.
Four lanes, one per shape, N = 5."""
import numpy as np
import pytest

from test_gpu_twin import solver, twin  # noqa: F401  (twin: the module's fixture of the twin)
from twin_bits_cases import (CASES, EDGE_DELAY_COLS, EDGE_T, K, as_bits, delay_edge_table, edge_index_times, inputs,
                             qp_inputs)

pytestmark = pytest.mark.gpu

N, TS = 5, 0.05


def same(a, b, what):
    """Equality of the 64-bit patterns: -0.0 is not +0.0, and a NaN equals only the same NaN."""
    a, b = as_bits(np.asarray(a)), as_bits(np.asarray(b))
    assert a.shape == b.shape and a.dtype.kind == b.dtype.kind, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a, b), f"{what}: {int((a != b).sum())} of {a.size} words differ"


def test_staging_edges_bit_identical(twin):
    from oracle.oracle import make_opts
    x0, _, sid = inputs()
    B, tab = len(x0), delay_edge_table()
    assert tab.shape == (B, EDGE_T, 6) and edge_index_times() == (1, EDGE_T, EDGE_T + 4)
    op = make_opts(N=N, sqp_iters=K)
    s = solver(N, B, sqp_iters=K)
    try:
        s.set_shape_ids(sid)
        s.set_reference_trajectories(tab)
        s.set_delay_comp(EDGE_DELAY_COLS * TS)
        assert s.delay_cols() == EDGE_DELAY_COLS
        for it in edge_index_times():
            s.controller_reset()                 # every step cold
            warm = twin.new_warm(B, N)
            u = s.controller_solve(x0, it)
            r = twin.controller_solve(op, x0, tab, it, warm, shape_id=sid, delay_cols=s.delay_cols())
            same(u, r["u0"], f"u0 (index_time {it})")
            for f in ("status", "sqp_iter", "qp_iter"):
                same(s.get(f), r[{"sqp_iter": "iters"}.get(f, f)], f"{f} (index_time {it})")
            same(s.get("x"), warm["X"], f"shifted X (index_time {it})")
            same(s.get("u"), warm["U"], f"shifted U (index_time {it})")
            same(s.get("pi"), warm["PI"], f"shifted PI (index_time {it})")
            same(s.get_cost(), r["cost"], f"cost (index_time {it})")
            assert not r["status"].any() and not s.get("status").any(), it
    finally:
        s.close()


@pytest.mark.parametrize("case,want", [("qp_n5_cap", [2, 2, 2, 2]), ("qp_n5_s0_out", [0, 3, 0, 0])])
def test_qp_status_codes_bit_identical(twin, case, want):
    from oracle.oracle import make_opts
    kw = dict(CASES[case])
    s0_out = kw.pop("s0_out", False)
    assert kw.pop("qp") and kw.pop("N") == N
    x0, traj, sid = inputs()
    B = len(x0)
    op = make_opts(N=N, sqp_iters=K, **kw)
    A, Bm, b, H, g, lo, hi, act, dx0 = qp_inputs(twin, op, x0, traj, sid, s0_out)
    s = solver(N, B, sqp_iters=K, **kw)
    try:
        r = s.qp_solve(A, Bm, b, H, g, lo, hi, dx0)
    finally:
        s.close()
    t = twin.qp(op, A, Bm, b, H, g, lo, hi, act, dx0)
    for k in ("dx", "du", "pi", "lam", "iters", "qp_status"):
        same(r[k], t[k], f"{case} {k}")
    assert r["qp_status"].tolist() == want and t["qp_status"].tolist() == want
