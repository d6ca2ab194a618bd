"""The IPM's loop-top sum with the predictor's barrier terms under it (qsp_solver.hip group_sum_over,
barrier_term, qp_ipm): only the schedule changed, so every output must equal the oracle's kernel-order
twin bit for bit, on all lanes.

What the change could break, and the case that shows it:
- the five-level fast path of the sum (16 < L <= 32 lanes per instance) against the general loop: L = 6,
  13 and 16 take the loop, L = 17, 21 and 32 the fast path (16 and 32 are its two edges); B = 385 leaves
  the last wave partly filled at two, three and four instances per wave;
- the barrier terms computed in front of the loop's exit test, once more than the factorisation needs
  them: qp_iters = 3 ends every QP at the cap (the extra pass follows a capped iteration), the
  library default 20 ends them by the stop test with instances of one wave leaving at different
  iterations (finished instances recompute the terms they hold), qp_mu_max = 1.2 makes QPs leave
  by the divergence exit (status 4);
- both loop forms (per-iteration launches and the fused loop), one and two stream parts, and the
  merit SQP's kernel, which holds the same qp_ipm.

Every case is two controller steps, a cold one and one warm-started from its shifted solution, B = 385,
K = 6.  The guards on the inputs (a lane with status 4 in each qp_mu_max case, every QP at the cap in each
qp_iters = 3 case, a wave of the warm step's first SQP iteration with unequal IPM counts in every other)
are asserted on the twin's own output, on the CPU, before the device is used.  Tolerance: none.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAMES = ("santal", "balea", "montana", "pulirapid")
B, K = 385, 6
# N: (stages per lane, lanes per instance, instances per wave)
LAYOUT = {5: (1, 6, 10), 12: (1, 13, 4), 15: (1, 16, 4), 20: (1, 21, 3), 31: (1, 32, 2), 33: (2, 17, 3)}
EXITS = {"default": {}, "cap3": dict(qp_iters=3), "mumax": dict(qp_mu_max=1.2)}


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


_REF = {}


def reference(N, nlp, exit_):
    """The twin's two controller steps of the case (cold, then warm-started from the shifted solution),
    computed once for all its variants and left unchanged.  A cold start's first QP takes the same six IPM
    iterations on every lane, so the wave with instances of different counts is looked for in the warm
    step's first SQP iteration, which is packed in lane order like every solve's first."""
    key = (N, nlp, exit_)
    if key in _REF:
        return _REF[key]
    from bench import straight_traj
    from oracle.oracle import Oracle, make_opts
    twin = Oracle(NAMES, twin=True)
    kw = EXITS[exit_]
    traj = straight_traj()
    x0, sid = inputs()
    op = make_opts(N=N, sqp_iters=K, nlp_mode=nlp, **kw)
    op1 = make_opts(N=N, sqp_iters=1, nlp_mode=nlp, **kw)
    warm = twin.new_warm(B, N)
    steps, first = [], []
    for step in range(2):
        w1 = {k: v.copy() for k, v in warm.items()}
        first.append(twin.controller_solve(op1, x0, traj, 1 + step, w1, shape_id=sid)["qp_iter"])
        r = twin.controller_solve(op, x0, traj, 1 + step, warm, shape_id=sid)
        r.update(X=warm["X"].copy(), U=warm["U"].copy(), PI=warm["PI"].copy())
        steps.append(r)
    # the guards, on the twin alone
    if exit_ == "mumax":
        assert (steps[0]["status"] == 4).sum() >= 1, f"N = {N}, nlp {nlp}: no lane with status 4 in the cold step"
    if exit_ == "cap3":
        # every QP ends at the cap
        for r in steps:
            assert np.all(r["qp_iter"] == 3 * K), f"N = {N}, nlp {nlp}: QPs below the cap"
    else:
        G = LAYOUT[N][2]
        q = first[1][:B // G * G].reshape(-1, G)
        assert np.any(q.min(1) != q.max(1)), f"N = {N}, nlp {nlp}: every wave's instances take the same IPM count"
    _REF[key] = dict(traj=traj, sid=sid, x0=x0, steps=steps)
    return _REF[key]


def run_case(monkeypatch, N, nlp, exit_, fused, parts):
    from uclv_qs_pushing_matlab_amd.objects import make_shape
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    ref = reference(N, nlp, exit_)
    if fused is not None:
        monkeypatch.setenv("QSP_FUSED_LOOP", fused)
    s = OcpSolver(N=N, batch=B, sqp_iters=K, nlp_solver_type="SQP" if nlp else "SQP_RTI", **EXITS[exit_])
    try:
        s.set_shapes([make_shape(n) for n in NAMES])
        s.set_shape_ids(ref["sid"])
        s.set_stream_parts(parts)
        assert tuple(s.layout()) == LAYOUT[N][:2]
        s.set_reference_trajectory(ref["traj"])
        for step, r in enumerate(ref["steps"]):
            u0 = s.controller_solve(ref["x0"], 1 + step)
            same(u0, r["u0"], f"u0 (step {step})")
            same(s.get("x"), r["X"], f"X (step {step})")
            same(s.get("u"), r["U"], f"U (step {step})")
            same(s.get("pi"), r["PI"], f"PI (step {step})")
            same(s.get("status"), r["status"], f"status (step {step})")
            same(s.get("qp_iter"), r["qp_iter"], f"qp_iter (step {step})")
            same(s.get("sqp_iter"), r["iters"], f"sqp_iter (step {step})")
    finally:
        s.close()


@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("exit_", list(EXITS))
@pytest.mark.parametrize("N", list(LAYOUT))
def test_sqp_rti_bit_identical(monkeypatch, N, exit_, fused):
    run_case(monkeypatch, N, 0, exit_, fused, 1)


@pytest.mark.parametrize("exit_", list(EXITS))
def test_two_stream_parts_bit_identical(monkeypatch, exit_):
    run_case(monkeypatch, 20, 0, exit_, "0", 2)


@pytest.mark.parametrize("exit_", list(EXITS))
@pytest.mark.parametrize("N", [12, 20])
def test_merit_sqp_bit_identical(monkeypatch, N, exit_):
    run_case(monkeypatch, N, 1, exit_, None, 1)
