"""GPU: non-finite and hopeless lanes inside the hardware the lanes of a batch share.

One wavefront holds 2 to 5 instances; they share the matrix-core factor steps, LDS record regions, the
DPP group sums and maxima, a wave-uniform interior-point loop and the packing sort.  Every test puts bad
lanes (tests/bad_lanes.py: their kinds, their placement on the waves, the status the rule of
include/qsp_nmpc.h gives them) into a healthy batch and compares three things, all bit for bit:
  * the mixed batch on the device against the twin: every lane, every output, NaN == NaN;
  * the healthy lanes of the mixed device run against a clean device run of the same batch --
    independently of the twin, which is isolated by construction (it runs lane after lane);
  * status and sqp_iter against the rule and against the literal restatement.
No input of these tests reaches an index: index_time and the shape ids are valid on every lane, the
spline's span guess (int)(sig * inv_h) is clamped before use (qsp_math.hpp), sin_cos reduces its
argument without an integer conversion (qsp_fp.hpp), the packing keys are clamped integers.
"""
import numpy as np
import pytest

import bad_lanes as bl
from conftest import straight_traj
from test_gpu_twin import NAMES, same, solver

pytestmark = pytest.mark.gpu

K = 5
COUNTS = ("status", "sqp_iter", "qp_iter", "qp_capped", "qp_stalled")


@pytest.fixture(scope="module")
def twin():
    from oracle.oracle import Oracle
    return Oracle(NAMES, twin=True)


@pytest.fixture(scope="module")
def literal():
    from oracle.oracle import Oracle
    return Oracle(NAMES)


def opts(N, nlp=0, K=K, **kw):
    from oracle.oracle import make_opts
    return make_opts(N=N, sqp_iters=K, nlp_mode=nlp, stages_per_lane=kw.get("stages_per_lane", 0),
                     factor_scan=int(kw.get("factor_scan", False)))


def outputs(s, u0):
    out = dict(u0=u0, X=s.get("x"), U=s.get("u"), PI=s.get("pi"), cost=s.get_cost())
    out.update({f: s.get(f) for f in COUNTS})
    return out


def twin_outputs(r, X, U, PI):
    out = dict(u0=r.get("u0", U[:, 0]), X=X, U=U, PI=PI, cost=r["cost"], sqp_iter=r["iters"])
    out.update({f: r[f] for f in COUNTS if f != "sqp_iter"})
    return out


def three_way(dev_mixed, dev_clean, twin_mixed, bad, what):
    for k in dev_mixed:
        same(dev_mixed[k], twin_mixed[k], f"{what}: device against twin, {k}")
    for k in dev_mixed:
        bl.healthy_equal(dev_mixed[k], dev_clean[k], bad, f"{what}: mixed against clean on the device, {k}")


def device_controller(N, nlp, b, which, **kw):
    s = solver(N, b["B"], sqp_iters=K, nlp_solver_type="SQP" if nlp else "SQP_RTI", **kw)
    try:
        s.set_shape_ids(b["sid"])
        s.set_reference_trajectories(b[which]["traj"])
        return outputs(s, s.controller_solve(b[which]["x0"], b["index"]))
    finally:
        s.close()


def controller_rounds(twin, literal, N, S, nlp=0, **kw):
    """Every round of the catalogue at this layout: one cold-start controller solve, three ways."""
    G = bl.instances_per_wave(N, S)
    op = opts(N, nlp, **kw)
    for rnd in range(bl.rounds(G)):
        b = bl.ctrl_batch(N, S, seed=3, rnd=rnd)
        assert b["G"] == G and b["B"] == 4 * G + 1
        dm, dc = device_controller(N, nlp, b, "mixed", **kw), device_controller(N, nlp, b, "clean", **kw)
        w = twin.new_warm(b["B"], N)
        r = twin.controller_solve(op, b["mixed"]["x0"], b["mixed"]["traj"], b["index"], w, shape_id=b["sid"])
        three_way(dm, dc, twin_outputs(r, w["X"], w["U"], w["PI"]), b["bad"], f"N {N} round {rnd}")
        bl.check_clean(dc["status"], b["bad"], merit=bool(nlp))
        np.testing.assert_array_equal(dm["status"], bl.rule_status(b["mixed"]["x0"], b["bad"], dc["status"]),
                                      err_msg=f"N {N} round {rnd}: status against the rule")
        ls, li = bl.literal_controller(literal, op, b["mixed"]["x0"], b["mixed"]["traj"], b["index"], b["sid"])
        np.testing.assert_array_equal(dm["status"], ls, err_msg=f"N {N} round {rnd}: status against the literal")
        np.testing.assert_array_equal(dm["sqp_iter"], li, err_msg=f"N {N} round {rnd}: sqp_iter against the literal")


@pytest.mark.parametrize("env", [("QSP_FUSED_LOOP", "0"), ("QSP_FUSED_LOOP", "1"), ("QSP_MFMA_WALK", "0")])
def test_three_instances_per_wave(twin, literal, monkeypatch, env):
    """N = 20: G = 3, the matrix-core factor walk (three instances on the four blocks of one
    v_mfma_f64_4x4x4), as per-iteration launches, as the fused small-batch loop, and with the lane walk in
    its place."""
    monkeypatch.setenv(*env)
    controller_rounds(twin, literal, 20, 1)


@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("N,S,scan", [(14, 1, False), (11, 1, False), (31, 1, False), (50, 2, False), (50, 2, True)])
def test_layouts(twin, literal, monkeypatch, N, S, scan, fused):
    """N = 14: G = 4, every matrix-core block a different instance; N = 11: G = 5, the lane walk;
    N = 31: G = 2; N = 50 at two stages per lane: G = 2, the walk and the factorisation scan."""
    monkeypatch.setenv("QSP_FUSED_LOOP", fused)
    kw = dict(stages_per_lane=S, factor_scan=True) if scan else dict(stages_per_lane=S)
    controller_rounds(twin, literal, N, S, **kw)


@pytest.mark.parametrize("N", [10, 20])
def test_merit_kernels(twin, literal, N):
    """nlp_solver_type 'SQP': the KKT test, the merit line search and the damped multiplier update next
    to a bad instance (at K = 5 the healthy lanes end at max_iter, status 2)."""
    controller_rounds(twin, literal, N, 1, nlp=1)


@pytest.mark.parametrize("nlp", [0, 1])
def test_acados_level_solve(twin, literal, nlp):
    """qsp_solve (set('constr_x0') ... solve()) at N = 20: a bad x0, y_ref or y_ref_e under a finite
    initial guess."""
    N, S = 20, 1
    G = bl.instances_per_wave(N, S)
    op = opts(N, nlp)
    for rnd in range(bl.rounds(G)):
        b = bl.ocp_batch(N, S, seed=7, rnd=rnd)

        def device(d):
            s = solver(N, b["B"], sqp_iters=K, nlp_solver_type="SQP" if nlp else "SQP_RTI")
            try:
                s.set_shape_ids(b["sid"])
                s.set("constr_x0", d["x0"])
                s.set("cost_y_ref", d["yref"])
                s.set("cost_y_ref_e", d["yref_e"])
                s.set("init_x", b["X"])
                s.set("init_u", b["U"])
                s.set("init_pi", np.zeros((b["B"], N, 4)))
                s.solve()
                return outputs(s, s.get("u")[:, 0])
            finally:
                s.close()
        dm, dc = device(b["mixed"]), device(b["clean"])
        run = lambda o, d: o.ocp_solve(op, d["x0"], d["yref"], d["yref_e"], b["X"], b["U"], shape_id=b["sid"])
        r = run(twin, b["mixed"])
        three_way(dm, dc, twin_outputs(r, r["X"], r["U"], r["PI"]), b["bad"], f"qsp_solve round {rnd}")
        bl.check_clean(dc["status"], b["bad"], merit=bool(nlp))
        np.testing.assert_array_equal(dm["status"], bl.rule_status(b["mixed"]["x0"], b["bad"], dc["status"]))
        rl = run(literal, b["mixed"])
        np.testing.assert_array_equal(dm["status"], rl["status"])
        np.testing.assert_array_equal(dm["sqp_iter"], rl["iters"])


@pytest.mark.parametrize("N,S,scan", [(20, 1, False), (20, 2, False), (50, 2, False), (50, 2, True)])
def test_qp_solve(twin, literal, N, S, scan):
    """qsp_qp_solve with one NaN per bad lane in g, A, b, lo or dx0: qp_status 1 on those lanes (their dx
    and du are non-finite), the other lanes' QPs untouched; and a NaN in H is no lane's data: the call is
    refused whole.  qsp_qp_solve takes the weights from lane 0's stage-0 and terminal entries of H and
    compares every other entry with them: a NaN in an entry that is only compared differs from them, a
    NaN in one that is read differs from itself."""
    from uclv_qs_pushing_matlab_amd import QspError
    kw = dict(stages_per_lane=S, factor_scan=scan)
    op = opts(N, **kw)
    G = bl.instances_per_wave(N, S)
    keys = ("dx", "du", "pi", "lam", "iters", "qp_status")
    for rnd in range(bl.rounds(G, bl.QP_KINDS)):
        b = bl.qp_batch(twin, op, rnd=rnd)
        s = solver(N, b["B"], **kw)
        try:
            assert s.layout()[0] == S
            dev = lambda d: s.qp_solve(*[d[k] for k in bl.QP_ARGS if k != "act"])
            dm, dc = dev(b["mixed"]), dev(b["clean"])
            if rnd == 0:
                # an entry that is only compared, then the entries that are read: lane 0's stage-0
                # state and input weights and its terminal weights
                for lane, col in ((int(np.flatnonzero(b["bad"])[0]), 6 * (N // 2) + 4), (0, 1), (0, 4), (0, 6 * N + 2)):
                    H = b["clean"]["H"].copy()
                    H[lane, col] = np.nan
                    with pytest.raises(QspError, match="Hessian"):
                        s.qp_solve(*[H if k == "H" else b["clean"][k] for k in bl.QP_ARGS if k != "act"])
        finally:
            s.close()
        t = twin.qp(op, *[b["mixed"][k] for k in bl.QP_ARGS])
        for k in keys:
            same(dm[k], t[k], f"qp round {rnd}: device against twin, {k}")
            bl.healthy_equal(dm[k], dc[k], b["bad"], f"qp round {rnd}: mixed against clean on the device, {k}")
        assert np.all(dc["qp_status"] == 0)
        np.testing.assert_array_equal(dm["qp_status"], np.where(b["bad"], 1, 0))
        np.testing.assert_array_equal(dm["qp_status"], literal.qp(op, *[b["mixed"][k] for k in bl.QP_ARGS])["qp_status"])


@pytest.mark.parametrize("delay", [0.0, 0.05])
def test_closed_loop_and_metrics(twin, literal, delay):
    """qsp_closed_loop and qsp_closed_loop_metrics, N = 10, T = 6, without and with one column of delay
    compensation: one lane's noise is NaN at step 2, another's 1e200 at step 3.  Status 1 resp. 4 from
    there on, every other lane as in the clean run; the metrics against their numpy restatement on the
    twin's trajectory, a bad lane's n_failed = T - its first bad step."""
    from closed_loop_metrics_ref import NAMES as METRIC_NAMES, closed_loop_metrics_ref
    N, T = 10, 6
    G = bl.instances_per_wave(N, 1)
    B = bl.batch_size(G)
    mixed_nz, clean_nz, bad, first = bl.closed_loop_noise(T, B, G)
    (a, ta), (c, tc) = sorted(first.items())
    x0, sid, traj = bl._x0(B, 3), np.arange(B) % 4, straight_traj()
    s = solver(N, B, sqp_iters=K)
    try:
        s.set_shape_ids(sid)
        s.set_reference_trajectory(traj)
        s.set_delay_comp(delay)
        D = s.delay_cols()
        assert D == (1 if delay else 0)
        res = {}
        for name, nz in (("mixed", mixed_nz), ("clean", clean_nz)):
            s.set_delay_comp(delay)          # zeroes the controller's input buffer: every run starts alike
            g = s.closed_loop(x0, T, noise=nz)
            s.set_delay_comp(delay)
            res[name] = (g, s.closed_loop_metrics(x0, T, noise=nz))
        s_lo, s_hi = s._lh[0], s._uh[0]
        op = opts(N)
        t = twin.closed_loop(op, x0, traj, T, shape_id=sid, noise=mixed_nz, delay_cols=D)
        modes = s.eval_modes(t["X"][:, :T].reshape(-1, 4), t["U"].reshape(-1, 2), shape_id=np.repeat(sid, T)).reshape(B, T)
    finally:
        s.close()
    (gm, mm), (gc, mc) = res["mixed"], res["clean"]
    for k in ("X", "Xsim", "U", "status"):
        same(gm[k], t[k], f"closed loop: device against twin, {k}")
        bl.healthy_equal(gm[k], gc[k], bad, f"closed loop: mixed against clean on the device, {k}")
    assert np.all(gc["status"] == 0)
    np.testing.assert_array_equal(gm["status"], bl.closed_loop_rule(gc["status"], first, {a: 1, c: 4}))
    np.testing.assert_array_equal(gm["status"], literal.closed_loop(op, x0, traj, T, shape_id=sid, noise=mixed_nz,
                                                                   delay_cols=D)["status"])
    with np.errstate(over="ignore"):     # the 1e200 lane's squared errors are +Inf on both sides
        ref = closed_loop_metrics_ref(t["X"], t["U"], t["status"], modes, traj, 1, s_lo, s_hi)
    for j, name in enumerate(METRIC_NAMES):
        np.testing.assert_array_equal(mm["metrics"][:, j], ref[:, j], err_msg=name)      # NaN == NaN
    for k in ("metrics", "x_end", "status"):
        bl.healthy_equal(mm[k], mc[k], bad, f"metrics: mixed against clean on the device, {k}")
    same(mm["x_end"], gm["X"][:, -1], "metrics x_end")
    same(mm["status"], gm["status"][:, -1], "metrics status")
    assert mm["n_failed"][a] == T - ta and mm["n_failed"][c] == T - tc and np.all(mm["n_failed"][~bad] == 0)
    assert np.isnan(mm["sum_exy2"][a]) and np.isfinite(mm["metrics"][~bad]).all()


@pytest.mark.parametrize("nlp", [0, 1])
def test_controller_sequence_recovers(twin, literal, nlp):
    """Controller steps 0 (clean), 1 (bad x0), 2 and 3 (clean) on one handle: the bad lanes' status is the
    rule's at step 1 and the clean sequence's again at step 2, with a finite warm start; the healthy lanes
    have the clean sequence's bits at every step."""
    N, S = 20, 1
    G = bl.instances_per_wave(N, S)
    op = opts(N, nlp)
    traj = straight_traj()
    for rnd in range(bl.rounds(G, bl.X0_KINDS)):
        b = bl.ctrl_batch(N, S, seed=3, kinds=bl.X0_KINDS, rnd=rnd)
        handles = [solver(N, b["B"], sqp_iters=K, nlp_solver_type="SQP" if nlp else "SQP_RTI") for _ in range(2)]
        try:
            for s in handles:
                s.set_shape_ids(b["sid"])
                s.set_reference_trajectory(traj)
            sm, sc = handles
            wt, wl = twin.new_warm(b["B"], N), literal.new_warm(b["B"], N)
            for step in range(4):
                xm = b["mixed"]["x0"] if step == 1 else b["clean"]["x0"]
                dm, dc = outputs(sm, sm.controller_solve(xm, 1 + step)), outputs(sc, sc.controller_solve(b["clean"]["x0"], 1 + step))
                r = twin.controller_solve(op, xm, traj, 1 + step, wt, shape_id=b["sid"])
                three_way(dm, dc, twin_outputs(r, wt["X"], wt["U"], wt["PI"]), b["bad"], f"round {rnd} step {step}")
                bl.check_clean(dc["status"], b["bad"], merit=bool(nlp))
                np.testing.assert_array_equal(dm["status"], bl.rule_status(xm, b["bad"] & (step == 1), dc["status"]),
                                              err_msg=f"round {rnd} step {step}: status against the rule")
                rl = literal.controller_solve(op, xm, traj, 1 + step, wl, shape_id=b["sid"])
                # the literal: every lane at fixed K; with the merit SQP every lane at steps 0 and 1 and
                # none later (a lane warm-started twice may meet tol in one formulation and miss it by
                # rounding in the other: lane 8 at step 3, tests/test_bad_lanes.py)
                if not (nlp and step >= 2):
                    np.testing.assert_array_equal(dm["status"], rl["status"], err_msg=f"round {rnd} step {step}")
                    np.testing.assert_array_equal(dm["sqp_iter"], rl["iters"], err_msg=f"round {rnd} step {step}")
                if step >= 2:
                    assert all(np.isfinite(dm[k]).all() for k in ("X", "U", "PI", "u0", "cost"))
        finally:
            for s in handles:
                s.close()


def test_packing_and_two_streams(twin, literal):
    """B = 8 192, N = 20, K = 8 (as test_qp_iters_beyond_packing_levels): the packing sort regroups the
    instances by their iteration counts before every SQP iteration, and the batch runs as two stream parts.
    About 1 % of the lanes are bad at seeded random positions, and one wave's three lanes are.  Per-lane
    reference tables, so that the NaN-reference kinds are among them: such a lane's QP fails at once, a
    failed instance keeps its packing record, and so it holds the count-0 key, the extreme of the sort,
    through all K iterations."""
    from conftest import config2_x0
    N, B, Kp, index = 20, 8192, 8, 1
    rng = np.random.default_rng(2024)
    bad = np.zeros(B, bool)
    bad[rng.choice(B, 82, replace=False)] = True
    bad[3 * 1717:3 * 1717 + 3] = True                   # one whole wave of G = 3
    x0c = config2_x0(B, 91)
    tabc = np.broadcast_to(straight_traj()[None, :index + N + 8], (B, index + N + 8, 6)).copy()
    x0m, tabm = x0c.copy(), tabc.copy()
    lanes = np.flatnonzero(bad)
    for j, i in enumerate(lanes):
        bl.poison(x0m, tabm, i, bl.KINDS[j % len(bl.KINDS)], N, index)
    assert len(lanes) >= len(bl.KINDS)
    sid = np.arange(B) % 4

    def device(x0, tab):
        s = solver(N, B, sqp_iters=Kp)
        try:
            s.set_shape_ids(sid)
            s.set_reference_trajectories(tab)
            out = outputs(s, s.controller_solve(x0, index))
            assert s.stream_parts() == 2
            return out
        finally:
            s.close()
    dm, dc = device(x0m, tabm), device(x0c, tabc)
    op = opts(N, K=Kp)
    w = twin.new_warm(B, N)
    r = twin.controller_solve(op, x0m, tabm, index, w, shape_id=sid)
    three_way(dm, dc, twin_outputs(r, w["X"], w["U"], w["PI"]), bad, "packing")
    bl.check_clean(dc["status"], bad)
    np.testing.assert_array_equal(dm["status"], bl.rule_status(x0m, bad, dc["status"]))
    ls, li = bl.literal_controller(literal, op, x0m[bad], tabm[bad], index, sid[bad])
    np.testing.assert_array_equal(dm["status"][bad], ls)
    np.testing.assert_array_equal(dm["sqp_iter"][bad], li)
    yr = np.zeros(B, bool)
    yr[lanes] = [bl.KINDS[j % len(bl.KINDS)].where != "x0" for j in range(len(lanes))]
    assert yr.sum() >= 3 and np.all(dm["sqp_iter"][yr] == 0)
