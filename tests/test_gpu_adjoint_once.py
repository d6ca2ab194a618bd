"""The dynamics multipliers once per solve: the fixed-K SQP's QP kernels store an adjoint record per
successful QP and the epilogue walks the recursion from the record of each instance's last successful
QP (qsp_solver.hip qp_adjoint_record / adjoint_from_record).  The checker is the oracle's kernel-order
twin, which forms PI after every QP as the library did before; every output is compared bit for bit.

What can go wrong shows on instances that stop in the middle of a solve: a diverged QP at SQP
iteration it >= 1 (status 4) must leave the multipliers of QP it - 1, and an instance without any
successful QP (the stage-0 s bound) must keep what PI held -- zeros on a cold handle, the last
solve's shifted multipliers on a warm one.  qp_mu_max = 1.2 makes some QPs diverge mid-solve: the
twin gives 14, 5, 2 and 3 such lanes at N = 5, 12, 20 and 33 for these inputs (asserted below on the
twin's own output).

Shapes: N = 5 (lane walk, ten instances per wave), 12 (the smallest matrix-core walk), 20, 33 (two
stages per lane); B = 384 is several waves at each; K = 6.  Both the per-iteration launches and the
fused loop, one and two stream parts.  Tolerance: none.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAMES = ("santal", "balea", "montana", "pulirapid")
B, K, MU_MAX = 384, 6, 1.2
HORIZONS = (5, 12, 20, 33)
S_OUT = 0.02                       # outside [lh_s, uh_s] = [-0.06, 0.011]: the stage-0 bound stops the lane
OUT_FIRST = (3, 129, 383)          # lanes that never solve a QP (cold handle: PI stays zero)
OUT_SECOND = (7, 150)              # ... and lanes stopped only in the second solve: they keep their warm PI


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    eq = (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else (a == b)
    if not eq.all():
        bad = np.argwhere(~eq)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {a.size} entries differ; first at {i}: gpu {a[i]!r} twin {b[i]!r}")


def inputs():
    rng = np.random.default_rng(7)
    x0 = np.stack([rng.uniform(-0.02, 0.04, B), rng.uniform(-0.04, 0.03, B),
                   np.deg2rad(rng.uniform(-25.0, 25.0, B)), rng.uniform(-0.058, 0.0105, B)], 1)
    return x0, (np.arange(B) % 4).astype(np.int32)


def ocp_inputs(N, x0, traj):
    yref = np.broadcast_to(traj[None, 1:1 + N], (B, N, 6)).copy()
    rng = np.random.default_rng(70 + N)
    X = np.repeat(x0[:, None], N + 1, 1)
    U = np.broadcast_to(np.array([0.005, 0.0]), (B, N, 2)).copy()
    PI = rng.normal(0, 1e-3, (B, N, 4))
    return yref, yref[:, -1, :4].copy(), X, U, PI


_REF = {}


def reference(N):
    """The twin's results at horizon N, computed once for all variants of the test and left unchanged:
    two controller steps (cold, then warm with two more lanes stopped by the stage-0 bound) and one
    acados-level solve."""
    if N in _REF:
        return _REF[N]
    from bench import straight_traj
    from oracle.oracle import Oracle, make_opts
    twin = Oracle(NAMES, twin=True)
    op = make_opts(N=N, sqp_iters=K, qp_mu_max=MU_MAX)
    traj = straight_traj()
    x0, sid = inputs()
    xa = x0.copy()
    xa[list(OUT_FIRST), 3] = S_OUT
    xb = xa.copy()
    xb[list(OUT_SECOND), 3] = S_OUT
    warm = twin.new_warm(B, N)
    steps = []
    for step, x in enumerate((xa, xb)):
        r = twin.controller_solve(op, x, traj, 1 + step, warm, shape_id=sid)
        r.update(X=warm["X"].copy(), U=warm["U"].copy(), PI=warm["PI"].copy())
        steps.append(r)
    # non-vacuity, on the twin's own output: QPs that diverge in the middle of a solve, none at the
    # first iteration; the stage-0 bound's lanes never iterate and keep PI
    r0, r1 = steps
    mid = (r0["status"] == 4) & (r0["iters"] >= 1) & (r0["iters"] < K)
    assert mid.sum() >= 1, f"N = {N}: no lane diverges mid-solve on the twin"
    out0 = np.zeros(B, bool)
    out0[list(OUT_FIRST)] = True
    assert np.all(r0["iters"][out0] == 0) and np.all(r0["status"][out0] != 0)
    assert not np.any((r0["iters"] == 0) & (r0["status"] != 0) & ~out0)
    assert np.all(r0["PI"][out0] == 0.0) and np.all(r1["PI"][out0] == 0.0)
    for l in OUT_SECOND:
        assert r0["status"][l] == 0 and r1["iters"][l] == 0 and r1["status"][l] != 0
        assert np.array_equal(r1["PI"][l], r0["PI"][l]) and np.any(r0["PI"][l] != 0.0)
    yref, ye, X, U, PI = ocp_inputs(N, x0, traj)
    ro = twin.ocp_solve(op, x0, yref, ye, X, U, PI, shape_id=sid)
    assert ((ro["status"] == 4) & (ro["iters"] >= 1) & (ro["iters"] < K)).sum() >= 1, f"N = {N}: ocp_solve"
    _REF[N] = dict(traj=traj, sid=sid, x=(xa, xb), steps=steps, x0=x0, ocp_in=(yref, ye, X, U, PI), ocp=ro)
    return _REF[N]


@pytest.mark.parametrize("fused,parts", [("0", 1), ("0", 2), ("1", 1)])
@pytest.mark.parametrize("N", HORIZONS)
def test_multipliers_once_per_solve_bit_identical(monkeypatch, N, fused, parts):
    from uclv_qs_pushing_matlab_amd.objects import make_shape
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    ref = reference(N)
    monkeypatch.setenv("QSP_FUSED_LOOP", fused)
    s = OcpSolver(N=N, batch=B, sqp_iters=K, qp_mu_max=MU_MAX)
    try:
        s.set_shapes([make_shape(n) for n in NAMES])
        s.set_shape_ids(ref["sid"])
        s.set_stream_parts(parts)
        assert s.layout()[0] == (2 if N == 33 else 1)
        # controller mode (shifted outputs): a cold solve, then one on the warm handle
        s.set_reference_trajectory(ref["traj"])
        for step, (x, r) in enumerate(zip(ref["x"], ref["steps"])):
            u0 = s.controller_solve(x, 1 + step)
            same(s.get("pi"), r["PI"], f"pi (step {step})")
            same(s.get("x"), r["X"], f"x (step {step})")
            same(s.get("u"), r["U"], f"u (step {step})")
            same(u0, r["u0"], f"u0 (step {step})")
            same(s.get("status"), r["status"], f"status (step {step})")
            same(s.get("sqp_iter"), r["iters"], f"sqp_iter (step {step})")
            same(s.get("qp_iter"), r["qp_iter"], f"qp_iter (step {step})")
        # acados-level solve (unshifted outputs) on the same handle
        yref, ye, X, U, PI = ref["ocp_in"]
        s.set("constr_x0", ref["x0"])
        s.set("cost_y_ref", yref)
        s.set("cost_y_ref_e", ye)
        s.set("init_x", X)
        s.set("init_u", U)
        s.set("init_pi", PI)
        s.solve()
        r = ref["ocp"]
        # (the library's PI output of an acados-level solve is defined from the first successful QP
        # on; the twin returns the initial guess before that)
        had_qp = ~((r["iters"] == 0) & (r["status"] != 0))
        same(s.get("pi")[had_qp], r["PI"][had_qp], "pi (ocp_solve)")
        same(s.get("x"), r["X"], "x (ocp_solve)")
        same(s.get("u"), r["U"], "u (ocp_solve)")
        same(s.get_u0(), r["U"][:, 0], "u0 (ocp_solve)")
        same(s.get("status"), r["status"], "status (ocp_solve)")
        same(s.get("sqp_iter"), r["iters"], "sqp_iter (ocp_solve)")
        same(s.get("qp_iter"), r["qp_iter"], "qp_iter (ocp_solve)")
    finally:
        s.close()
