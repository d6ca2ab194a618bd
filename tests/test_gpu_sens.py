"""GPU: the solution sensitivities du_k/dx0 -- qsp_qp_sens (the walk on caller-given QP data), qsp_eval_sens /
qsp_eval_sens_device (an NLP point against the OCP) and qsp_get_sens (the last solve's iterate).

What must hold exactly is compared bit for bit: qsp_qp_sens against the host program of tests/test_sens_host.py
(the same header, contraction off on both sides), qsp_eval_sens against qsp_qp_sens fed qsp_eval_rk4's A_k, B_k
and the same diagonal (which holds the linearisation kernel, the workspace layout and the stage indexing to the
QP-level path), the device entry against the host entry, lanes beside a non-finite lane against the clean call,
qsp_get_sens against qsp_eval_sens of the handle's own iterate.  The accuracy of the walk itself is the host
test's subject (against a dense KKT solve); here the difference quotients of qsp_qp_solve are one more
independent check, with the bound of test_difference_quotients."""
import ctypes as C

import numpy as np
import pytest

import host_program
import manufactured_qp as mq
import point_cases
import sens_ref
from conftest import config2_x0, straight_traj
from point_cases import same_bits

pytestmark = pytest.mark.gpu

NAMES = ("santal", "balea")
ERR_ARG, ERR_STATE = r"\(-1\)", r"\(-3\)"
ALL = ("K0", "K", "dU", "P0", "flag")


def assert_same(got, want, lanes=slice(None), what=""):
    for k in want:
        if k in got:
            assert same_bits(got[k][lanes], want[k][lanes]), (what, k, np.abs(got[k][lanes] - want[k][lanes]).max())


make_solver = lambda N, B, **kw: point_cases.make_solver(N, B, NAMES, (np.arange(B) * 7 // 3) % 2, **kw)   # mixed per lane
nlp_point = lambda s, sid, seed: point_cases.nlp_point(s, sid, seed, feasible=True)


def rk4_data(s, sid, d):
    B, N = s.B, s.N
    _, A, Bm = s.eval_rk4(d["X"][:, :N].reshape(-1, 4), d["U"].reshape(-1, 2), shape_id=np.repeat(sid, N))
    return A.reshape(B, N, 4, 4), Bm.reshape(B, N, 4, 2)


# ------------------------------------------------------------------ test 1
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return host_program.build("sens_main", tmp_path_factory.mktemp("sens") / "sens_main", sanitize=False)


@pytest.mark.parametrize("N", [3, 20])
def test_qp_sens_is_the_host_walk(host_exe, tmp_path, N):
    """qsp_qp_sens on the host test's batches (their first 7 lanes are its 7), every output and every lane bit for
    bit the host program's; nb = 1 (one thread), 7, and 65 (a partial second wave and workgroup)."""
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    q = mq.make_batch("Fall", N, 65, 1)
    s = OcpSolver(N=5, batch=1)           # the QP's horizon is the call's, not the handle's
    try:
        for pattern in ("mixed", "inputs"):
            H, _ = sens_ref.barrier_H(q, 1, s_pins=(pattern == "mixed"))
            want = sens_ref.run_host_program(host_exe, tmp_path / "q.bin", q["A"], q["B"], H)
            assert not want["flag"].any() and all(np.isfinite(want[k]).all() for k in sens_ref.OUTPUTS)
            for nb in (1, 7, 65):
                got = s.qp_sens(q["A"][:nb].reshape(nb, N, 16), q["B"][:nb].reshape(nb, N, 8), H[:nb], want=ALL)
                assert_same(got, {k: v[:nb] for k, v in want.items()}, what=(pattern, nb))
            # K0 alone (no forward pass, no K store) has the same bits
            got = s.qp_sens(q["A"].reshape(65, N, 16), q["B"].reshape(65, N, 8), H)
            assert set(got) == {"K0"} and same_bits(got["K0"], want["K0"])
    finally:
        s.close()


# ------------------------------------------------------------------ test 2
@pytest.mark.parametrize("s0", [0, 1])
@pytest.mark.parametrize("N", [3, 20])
def test_eval_sens_is_qp_sens_of_its_own_stage_data(N, s0):
    B = 65
    s, sid = make_solver(N, B, stage0_s_bound=bool(s0))
    try:
        d = nlp_point(s, sid, 5 + N)
        A, Bm = rk4_data(s, sid, d)
        tau = s.Ts
        s.set("cost_y_ref", d["yref"])
        s.set("cost_y_ref_e", d["yref_e"])
        zero = np.zeros((B, N, 6))
        imp = sens_ref.implied_lam(d["X"], d["U"], d["PI"], d["yref"], A, Bm, s._W, tau)
        assert (imp[:, :, 2:] > 0).any() and (imp[:, 1:, :2] > 0).any() and not imp[:, 0, :2].any()
        for name, kw, lam, t_floor in (("given LAM, PI = 0", dict(PI=np.zeros((B, N, 4)), LAM=d["LAM"]), d["LAM"], 1e-8),
                                       ("given LAM, t_floor 1e-3", dict(LAM=d["LAM"]), d["LAM"], 1e-3),
                                       ("implied", dict(PI=d["PI"]), imp, 1e-8),
                                       ("no multipliers", dict(), zero, 1e-8)):
            got = s.eval_sens(d["X"], d["U"], t_floor=t_floor, want=ALL, **kw)
            H = sens_ref.nlp_H(d["X"], d["U"], lam, s._W, s._We, tau, s._lh, s._uh, s0, t_floor)
            want = s.qp_sens(A.reshape(B, N, 16), Bm.reshape(B, N, 8), H, want=ALL)
            assert not want["flag"].any() and np.isfinite(want["dU"]).all()
            assert_same(got, want, what=name)
        # the option overrides the handle's stage0_s_bound
        got = s.eval_sens(d["X"], d["U"], LAM=d["LAM"], want=ALL, s0_bound=not s0)
        H = sens_ref.nlp_H(d["X"], d["U"], d["LAM"], s._W, s._We, tau, s._lh, s._uh, not s0, 1e-8)
        assert_same(got, s.qp_sens(A.reshape(B, N, 16), Bm.reshape(B, N, 8), H, want=ALL), what="s0_bound option")
        assert d["LAM"][:, 0, :2].any()
        # x0 stands for X's row 0
        xa = config2_x0(B, 99)
        X2 = d["X"].copy()
        X2[:, 0] = xa
        assert_same(s.eval_sens(d["X"], d["U"], LAM=d["LAM"], x0=xa, want=ALL),
                    s.eval_sens(X2, d["U"], LAM=d["LAM"], want=ALL), what="x0")
    finally:
        s.close()


# ------------------------------------------------------------------ test 3
def test_difference_quotients_of_qp_solve():
    """(du(dx0 + delta e_j) - du(dx0 - delta e_j)) / (2 delta) of qsp_qp_solve, delta = 1e-6, against qsp_qp_sens
    with d = lam / slack of the solve's own answer at delta = 0: manufactured QPs with strict complementarity
    (family Fu: active input bounds, multipliers in [0.1, 5]), N = 5, nb = 16.  The interior point's stop
    tolerance, not the kernel, sets the floor, so the bound is 4 x what the CPU twin's own quotients miss the
    dense sensitivity (tests/sens_ref.py) by on the same batch: 7.03e-8 measured (tests/test_sens_api.py keeps that
    figure), bound 2.84e-7, at sensitivities up to 1.96.  QPs whose active set differs between the solves are
    left out, at most 2 of 16 (the twin leaves out none)."""
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    c = sens_ref.QUOT
    N, nb = c["N"], c["nb"]
    q = mq.make_batch(c["family"], N, nb, c["seed"])
    s = OcpSolver(N=N, batch=1, qp_iters=mq.QP_ITERS, mu_stop=mq.MU_STOP, stage0_s_bound=False)
    try:
        A16, B8 = q["A"].reshape(nb, N, 16), q["B"].reshape(nb, N, 8)
        solve = lambda dx0: s.qp_solve(A16, B8, q["b"], q["H"], q["g"], q["lo"], q["hi"], dx0)
        Q, H, keep = sens_ref.quotient_check(solve, q, c["delta"])
        got = s.qp_sens(A16, B8, H, want=("dU", "flag"))
    finally:
        s.close()
    err = np.abs(Q - got["dU"]).reshape(nb, -1).max(1)
    print("kept %d of %d; worst |quotient - dU| %.3e (bound %.3e); max |dU| %.2f"
          % (keep.sum(), nb, err[keep].max(), 4 * c["twin_err"], np.abs(got["dU"]).max()))
    assert not got["flag"].any()
    assert keep.sum() >= nb - c["max_left_out"]
    assert np.all(err[keep] <= 4 * c["twin_err"]), err


# ------------------------------------------------------------------ test 4
def test_device_entry_and_optional_outputs():
    import torch
    from uclv_qs_pushing_matlab_amd._lib import SensIO
    N, B = 20, 65
    s, sid = make_solver(N, B)
    try:
        d = nlp_point(s, sid, 31)
        want = s.eval_sens(d["X"], d["U"], PI=d["PI"], LAM=d["LAM"], want=ALL)
        dev = torch.device("cuda", 0)
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
        ins = dict(X=t(d["X"]), U=t(d["U"]), PI=t(d["PI"]), LAM=t(d["LAM"]), shape_id=t(np.asarray(sid, np.int32)))
        CANARY = -7.25
        shapes = dict(K0=(B, 2, 4), K=(B, N, 2, 4), dU=(B, N, 2, 4), P0=(B, 10))

        def run(names):
            outs = {k: torch.full(sh, CANARY, dtype=torch.float64, device=dev) for k, sh in shapes.items()}
            outs["flag"] = torch.full((B,), 77, dtype=torch.int32, device=dev)
            io = SensIO()
            for k, v in ins.items():
                setattr(io, k, v.data_ptr())
            for k in names:
                setattr(io, k, outs[k].data_ptr())
            torch.cuda.synchronize()          # the tensors are filled before the handle's stream reads them
            s.eval_sens_device(io)
            s.synchronize()
            return {k: v.cpu().numpy() for k, v in outs.items()}

        got = run(ALL)
        assert_same(got, want, what="device entry")
        # NULL optional outputs are not written: the buffers beside them keep their fill
        got = run(("K0", "P0"))
        assert same_bits(got["K0"], want["K0"]) and same_bits(got["P0"], want["P0"])
        assert np.all(got["K"] == CANARY) and np.all(got["dU"] == CANARY) and np.all(got["flag"] == 77)
        got = run(("K0", "dU"))
        assert same_bits(got["dU"], want["dU"]) and np.all(got["K"] == CANARY) and np.all(got["P0"] == CANARY)
        # implied multipliers: the references given with the call are the ones the host entry takes from the handle
        s.set("cost_y_ref", d["yref"])
        s.set("cost_y_ref_e", d["yref_e"])
        want = s.eval_sens(d["X"], d["U"], PI=d["PI"], want=ALL)
        assert not same_bits(want["K0"], got["K0"])
        del ins["LAM"]
        ins["yref"] = t(d["yref"] + 0.0)
        assert_same(run(ALL), want, what="device entry, implied multipliers")
    finally:
        s.close()


# ------------------------------------------------------------------ test 5
def test_bad_lanes():
    N, B = 20, 65
    s, sid = make_solver(N, B)
    try:
        d = nlp_point(s, sid, 41)
        want = s.eval_sens(d["X"], d["U"], LAM=d["LAM"], want=ALL)
        assert not want["flag"].any() and all(np.isfinite(want[k]).all() for k in sens_ref.OUTPUTS)
        X, LAM = d["X"].copy(), d["LAM"].copy()
        X[3, 7, 2] = np.nan
        LAM[40, N - 1, 5] = np.inf
        got = s.eval_sens(X, d["U"], LAM=LAM, want=ALL)
        bad = [3, 40]
        good = np.setdiff1d(np.arange(B), bad)
        for k in sens_ref.OUTPUTS:
            assert np.all(np.isnan(got[k][bad])), (k, got[k][bad])
        assert np.all(got["flag"][bad] == 1) and not got["flag"][good].any()
        assert_same(got, want, lanes=good, what="beside bad lanes")
        # the last row of X counts too, though nothing is computed from it
        X = d["X"].copy()
        X[64, N, 0] = np.nan
        got = s.eval_sens(X, d["U"], LAM=d["LAM"], want=ALL)
        assert got["flag"][64] == 1 and np.all(np.isnan(got["K0"][64])) and not got["flag"][:64].any()
        assert_same(got, want, lanes=np.arange(64), what="beside the last lane")
        # the QP-level entry: a NaN in B of lane 3, an Inf in H of lane 40
        A, Bm = rk4_data(s, sid, d)
        H = sens_ref.nlp_H(d["X"], d["U"], d["LAM"], s._W, s._We, s.Ts, s._lh, s._uh, 1, 1e-8)
        H[40, 6 * 5 + 4] = np.inf
        Bm[3, 11, 2, 1] = np.nan
        got = s.qp_sens(A.reshape(B, N, 16), Bm.reshape(B, N, 8), H, want=ALL)
        for k in sens_ref.OUTPUTS:
            assert np.all(np.isnan(got[k][bad])), (k, got[k][bad])
        assert np.all(got["flag"][bad] == 1) and not got["flag"][good].any()
        assert_same(got, want, lanes=good, what="qp_sens beside bad lanes")
    finally:
        s.close()


# ------------------------------------------------------------------ test 6
@pytest.mark.parametrize("mode", ["SQP_RTI", "SQP"])
def test_get_sens_is_eval_sens_of_the_iterate(mode):
    from uclv_qs_pushing_matlab_amd import _lib
    N, B = 20, 64
    s, sid = make_solver(N, B, sqp_iters=30, nlp_solver_type=mode)
    try:
        with pytest.raises(_lib.QspError, match=ERR_STATE):
            s.get_sens()
        point_cases.cold_solve(s, 21)
        got = s.get_sens(want=ALL)
        lam = s.get("lam") if mode == "SQP" else None
        want = s.eval_sens(s.get("x"), s.get("u"), PI=s.get("pi"), LAM=lam, want=ALL)
        assert_same(got, want, what=mode)
        ok = s.get("status") == 0
        assert ok.sum() >= 10 and not got["flag"][ok].any()
        assert same_bits(s.get("sens_K0"), got["K0"])
        k0 = np.abs(got["K0"][ok]).reshape(ok.sum(), -1).max(1)
        print("%s: status 0 on %d lanes; max |K0| over them: median %.3g, largest %.3g" % (mode, ok.sum(), np.median(k0), k0.max()))
    finally:
        s.close()


@pytest.mark.parametrize("mode", ["SQP_RTI", "SQP"])
def test_get_sens_after_a_controller_step(mode):
    """After qsp_controller_solve the getters return the warm start shifted by one stage.  With 'SQP' the step's
    own iterate and bound multipliers are still on the handle and qsp_get_sens answers from them: the stage gains
    K_k, k >= 1, depend on stages k .. N only, which the shifted getters still show (row k of the iterate is their
    row k - 1), so they must equal eval_sens of the iterate put back together, bit for bit.  With 'SQP_RTI' the
    unshifted dynamics multipliers are gone and the call says so."""
    from uclv_qs_pushing_matlab_amd import _lib
    N, B = 20, 64
    s, sid = make_solver(N, B, sqp_iters=30, nlp_solver_type=mode)
    try:
        s.set_reference_trajectory(straight_traj())
        x0 = config2_x0(B, 23)
        u0 = s.controller_solve(x0, 1)
        if mode == "SQP_RTI":
            with pytest.raises(_lib.QspError, match=ERR_STATE):
                s.get_sens()
            return
        got = s.get_sens(want=ALL)
        Xs, Us, lam = s.get("x"), s.get("u"), s.get("lam")
        X = np.concatenate([x0[:, None], Xs[:, :N]], 1)          # row 0: any finite state (K_k, k >= 1, do not see it)
        U = np.concatenate([u0[:, None], Us[:, :N - 1]], 1)
        want = s.eval_sens(X, U, LAM=lam, want=ALL)
        assert same_bits(got["K"][:, 1:], want["K"][:, 1:])
        ok = s.get("status") == 0
        assert ok.sum() >= 10 and not got["flag"][ok].any() and np.isfinite(got["K0"][ok]).all()
    finally:
        s.close()


# ------------------------------------------------------------------ test 7
def test_argument_errors():
    from uclv_qs_pushing_matlab_amd import _lib
    from uclv_qs_pushing_matlab_amd._lib import ptr
    from uclv_qs_pushing_matlab_amd.objects import make_shape
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    N, B = 3, 4
    z = lambda *sh: np.zeros(sh)
    s = OcpSolver(N=N, batch=B)
    try:
        X, U = z(B, N + 1, 4), z(B, N, 2)
        with pytest.raises(_lib.QspError, match=ERR_STATE):          # no shapes
            s.eval_sens(X, U)
        s.set_shapes([make_shape(n) for n in NAMES], shape_id=np.arange(B) % 2)
        assert set(s.eval_sens(X, U)) == {"K0"}
        for t_floor in (0.0, -1e-8, np.nan, np.inf):
            with pytest.raises(_lib.QspError, match=ERR_ARG):
                s.eval_sens(X, U, t_floor=t_floor)
        with pytest.raises(_lib.QspError, match=ERR_STATE):          # implied multipliers without references
            s.eval_sens(X, U, PI=z(B, N, 4))
        L, h = s._L, s.handle
        o = _lib.SensOpts()
        L.qsp_default_sens_opts(C.byref(o))
        assert o.struct_size == C.sizeof(_lib.SensOpts) and o.t_floor == 1e-8 and o.s0_bound == -1
        K0 = z(B, 2, 4)
        assert L.qsp_eval_sens(h, C.byref(o), None, ptr(X), ptr(U), None, None, ptr(K0), None, None, None, None) == 0
        assert L.qsp_eval_sens(h, None, None, ptr(X), ptr(U), None, None, ptr(K0), None, None, None, None) == 0
        assert L.qsp_eval_sens(h, C.byref(o), None, ptr(X), ptr(U), None, None, None, None, None, None, None) == -1
        assert L.qsp_eval_sens(h, C.byref(o), None, None, ptr(U), None, None, ptr(K0), None, None, None, None) == -1
        assert L.qsp_eval_sens(h, C.byref(o), None, ptr(X), None, None, None, ptr(K0), None, None, None, None) == -1
        assert L.qsp_eval_sens(None, C.byref(o), None, ptr(X), ptr(U), None, None, ptr(K0), None, None, None, None) == -1
        assert L.qsp_eval_sens_device(h, C.byref(o), None, None) == -1
        assert L.qsp_eval_sens_device(h, C.byref(o), C.byref(_lib.SensIO()), None) == -1
        assert L.qsp_get_sens(h, C.byref(o), None, None, None, None, None) == -1
        o.struct_size += 8
        assert L.qsp_eval_sens(h, C.byref(o), None, ptr(X), ptr(U), None, None, ptr(K0), None, None, None, None) == -1
        o.struct_size -= 8
        o.s0_bound = 2
        assert L.qsp_eval_sens(h, C.byref(o), None, ptr(X), ptr(U), None, None, ptr(K0), None, None, None, None) == -1
        # qsp_qp_sens: null pointers, sizes, and an A outside the accepted structure
        q = mq.make_batch("F0", N, 2, 1)
        A, Bq, H = q["A"].reshape(2, N, 16).copy(), q["B"].reshape(2, N, 8).copy(), q["H"].copy()
        K0 = z(2, 2, 4)
        assert L.qsp_qp_sens(h, 2, N, ptr(A), ptr(Bq), ptr(H), ptr(K0), None, None, None, None) == 0
        for args in ((None, Bq, H, K0), (A, None, H, K0), (A, Bq, None, K0), (A, Bq, H, None)):
            assert L.qsp_qp_sens(h, 2, N, *[None if a is None else ptr(a) for a in args], None, None, None, None) == -1
        assert L.qsp_qp_sens(h, 0, N, ptr(A), ptr(Bq), ptr(H), ptr(K0), None, None, None, None) == -1
        assert L.qsp_qp_sens(h, 2, 0, ptr(A), ptr(Bq), ptr(H), ptr(K0), None, None, None, None) == -1
        for idx, val in ((4, 0.1), (0, 1.5), (14, -0.2), (10, np.nan)):      # a10, a00, a32, a22
            A2 = A.copy()
            A2[1, N - 1, idx] = val
            with pytest.raises(_lib.QspError, match=ERR_ARG):
                s.qp_sens(A2, Bq, H)
    finally:
        s.close()
