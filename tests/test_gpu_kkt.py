"""GPU: the KKT evaluators -- qsp_eval_kkt / qsp_eval_kkt_device (an NLP iterate against the OCP) and
qsp_qp_residuals (a QP point against caller-given data), with qsp_get_lam.

Comparisons against numpy use the derived bound of tests/kkt_ref.py, |got - ref| <= 64 eps * term scale
(each test prints its worst ratio); for the NLP the reference takes xn, A, B from OcpSolver.eval_rk4 at the
same points -- the same device arithmetic -- so only the residual arithmetic is under test.  What must hold
exactly is compared bit for bit: res and parts against the maxima of stage_res, the device entry against
the host entry, lanes beside a non-finite lane against the clean call, and on the merit SQP's converged
lanes the evaluator against the solver's own last test (get('residuals')): both run kkt_stage on rk4<true>
of the same point with the same multipliers, and maxima are order-free."""
import ctypes as C

import numpy as np
import pytest

import kkt_ref
import manufactured_qp as mq
import point_cases
from point_cases import same_bits

pytestmark = pytest.mark.gpu

NAMES = ("santal", "balea", "montana", "pulirapid")
ERR_ARG, ERR_STATE = r"\(-1\)", r"\(-3\)"


def within(got, ref, scale, extra=0.0):
    return np.all(np.abs(got - ref) <= kkt_ref.BOUND * scale + extra)


make_solver = lambda N, B, **kw: point_cases.make_solver(N, B, NAMES, np.arange(B) % 4, **kw)
nlp_inputs = lambda s, sid, seed: point_cases.nlp_point(s, sid, seed, feasible=False)


def nlp_reference(s, sid, d, lam, x0):
    B, N = s.B, s.N
    xn, A, Bm = s.eval_rk4(d["X"][:, :N].reshape(-1, 4), d["U"].reshape(-1, 2), shape_id=np.repeat(sid, N))
    return kkt_ref.nlp_residuals(d["X"], d["U"], d["PI"], lam, d["yref"], d["yref_e"], xn.reshape(B, N, 4),
                                 A.reshape(B, N, 4, 4), Bm.reshape(B, N, 4, 2), s.Ts, s._W, s._We, s._lh, s._uh,
                                 bool(s.opts.stage0_s_bound), x0=x0)


def eval_device(s, d, lam, x0, sid=None):
    """eval_kkt through qsp_eval_kkt_device on torch tensors."""
    import torch
    from uclv_qs_pushing_matlab_amd._lib import KKT_PARTS, KktIO
    dev = torch.device("cuda", 0)
    t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev)
    ins = {k: t(v) for k, v in (("x0", x0), ("X", d["X"]), ("U", d["U"]), ("PI", d["PI"]), ("LAM", lam),
                                ("yref", d["yref"]), ("yref_e", d["yref_e"]),
                                ("shape_id", None if sid is None else np.asarray(sid, np.int32)))}
    outs = dict(res=torch.zeros((s.B, 4), dtype=torch.float64, device=dev),
                parts=torch.zeros((s.B, len(KKT_PARTS)), dtype=torch.float64, device=dev),
                stage_res=torch.zeros((s.B, s.N + 1, 4), dtype=torch.float64, device=dev))
    io = KktIO()
    for k, v in list(ins.items()) + list(outs.items()):
        setattr(io, k, None if v is None else v.data_ptr())
    torch.cuda.synchronize()          # the tensors are filled before the handle's stream reads them
    s.eval_kkt_device(io)
    s.synchronize()
    return tuple(outs[k].cpu().numpy() for k in ("res", "parts", "stage_res"))


# ------------------------------------------------------------------ test 2
@pytest.mark.parametrize("family", ["F0", "Fall"])
@pytest.mark.parametrize("N", [3, 20, 70])
def test_qp_residuals(N, family):
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    nb = 70
    q = mq.make_batch(family, N, nb, 1)
    exact = (q["dx"], q["du"], q["pi"], q["lam"])
    rng = np.random.default_rng(11)
    pert = tuple(a + 1e-3 * rng.uniform(-1, 1, a.shape) for a in exact)
    qi = mq.make_batch("F0", N, nb, 1, stage0_infeasible=True)
    worst = 0.0
    for s0 in (False, True):
        s = OcpSolver(N=N, batch=1, stage0_s_bound=s0)
        try:
            data = [q[k].reshape(nb, N, -1) if k in ("A", "B") else q[k] for k in ("A", "B", "b", "H", "g", "lo", "hi", "dx0")]
            got = s.qp_residuals(*data, *exact)
            _, scale = kkt_ref.qp_residuals(q, *exact, s0)
            for k in kkt_ref.QP_KEYS:
                worst = max(worst, kkt_ref.worst_ratio(got[k], 0.0, scale[k]))
                assert within(got[k], 0.0, scale[k]), (s0, k, got[k])
            got = s.qp_residuals(*data, *pert)
            ref, scale = kkt_ref.qp_residuals(q, *pert, s0)
            for k in kkt_ref.QP_KEYS:
                worst = max(worst, kkt_ref.worst_ratio(got[k], ref[k], scale[k]))
                assert within(got[k], ref[k], scale[k]), (s0, k, got[k], ref[k])
            assert got["stat_u"].min() > 1e-5 and got["dyn"].min() > 1e-5
            if not s0:   # the row off and its multipliers zero: tests/manufactured_qp.py::kkt_residuals
                lam = pert[3].copy()
                lam[:, 0, :2] = 0.0
                got = s.qp_residuals(*data, *pert[:3], lam)
                ref = mq.kkt_residuals(q, *pert[:3], lam)
                _, scale = kkt_ref.qp_residuals(q, *pert[:3], lam, 0)
                for k in kkt_ref.QP_KEYS:
                    worst = max(worst, kkt_ref.worst_ratio(got[k], ref[k], scale[k]))
                    assert within(got[k], ref[k], scale[k]), (k, got[k], ref[k])
            # the stage-0 s outside its bound: counted with the row on, no row of the problem with it off
            datai = [qi[k].reshape(nb, N, -1) if k in ("A", "B") else qi[k] for k in ("A", "B", "b", "H", "g", "lo", "hi", "dx0")]
            gi = s.qp_residuals(*datai, qi["dx"], qi["du"], qi["pi"], qi["lam"])
            _, scale = kkt_ref.qp_residuals(qi, qi["dx"], qi["du"], qi["pi"], qi["lam"], s0)
            if s0:
                assert np.all(gi["infeas"] > 0.09), gi["infeas"]
            else:
                assert within(gi["infeas"], 0.0, scale["infeas"]), gi["infeas"]
        finally:
            s.close()
    print("N = %d %s: worst |got - ref| / (64 eps term scale) = %.3f" % (N, family, worst))


# ------------------------------------------------------------------ test 3
@pytest.mark.parametrize("B", [1, 70])
@pytest.mark.parametrize("N", [3, 20, 70])
def test_eval_kkt_against_numpy(N, B):
    s, sid = make_solver(N, B, stage0_s_bound=(B == 70))    # both values of the stage-0 s row
    try:
        d = nlp_inputs(s, sid, 3 + N)
        worst = {}
        for mode, lam in (("given", d["LAM"]), ("implied", None)):
            r = nlp_reference(s, sid, d, lam, d["x0"])
            res, parts, sres = s.eval_kkt(d["X"], d["U"], d["PI"], "implied" if lam is None else lam, x0=d["x0"],
                                          yref=d["yref"], yref_e=d["yref_e"], parts=True, stages=True)
            ex = r["comp_extra"]
            tol_s, tol_p, tol_r = np.zeros_like(sres), np.zeros_like(parts), np.zeros_like(res)
            tol_s[..., 3], tol_p[:, 6], tol_r[:, 3] = ex, ex.max(1), ex.max(1)
            for name, got, ref, scale, tol in (("stage_res", sres, r["stage_res"], r["stage_res_scale"], tol_s),
                                               ("parts", parts, r["parts"], r["parts_scale"], tol_p),
                                               ("res", res, r["res"], r["res_scale"], tol_r)):
                worst[mode, name] = kkt_ref.worst_ratio(got, ref, scale + tol / kkt_ref.BOUND)
                assert within(got, ref, scale, tol), (mode, name, np.abs(got - ref).max())
            assert np.all(res[:, :2] > 0.0) and np.all(np.isfinite(sres))
            if lam is None:     # implied multipliers: the bounded components' stationarity is zero
                assert np.all(parts[:, 0] == 0.0) and np.all(res[:, 3] > 0.0)
            # res and parts are the maxima of stage_res, bit for bit
            mx = sres.max(1)
            assert same_bits(res, mx)
            assert same_bits(parts[:, :3].max(1), mx[:, 0]) and same_bits(parts[:, 3:5].max(1), mx[:, 1])
            assert same_bits(parts[:, 5:], mx[:, 2:])
            # x0 = X_0 adds nothing
            a = s.eval_kkt(d["X"], d["U"], d["PI"], "implied" if lam is None else lam, x0=d["X"][:, 0],
                           yref=d["yref"], yref_e=d["yref_e"])
            b = s.eval_kkt(d["X"], d["U"], d["PI"], "implied" if lam is None else lam, yref=d["yref"], yref_e=d["yref_e"])
            assert same_bits(a, b)
            assert np.all(res[:, 1] >= b[:, 1])
            # the device entry on caller-owned buffers
            dres, dparts, dsres = eval_device(s, d, lam, d["x0"], sid)
            assert same_bits(dres, res) and same_bits(dparts, parts) and same_bits(dsres, sres)
        print("N = %d B = %d: worst |got - ref| / bound: %s" % (N, B, {k: "%.3f" % v for k, v in worst.items()}))
    finally:
        s.close()


# ------------------------------------------------------------------ test 4
def test_reproduces_the_merit_sqp_test():
    N, nb, K = 20, 64, 30
    s, sid = make_solver(N, nb, sqp_iters=K, nlp_solver_type="SQP")
    try:
        point_cases.cold_solve(s, 21)
        conv = np.nonzero(s.get("status") == 0)[0]
        assert len(conv) >= 10, len(conv)
        want = s.get("residuals")
        got = s.eval_kkt(s.get("x"), s.get("u"), s.get("pi"), s.get("lam"))
        print("converged lanes: %d; largest residuals there: %s" % (len(conv), want[conv].max(0)))
        assert np.all(want[conv][:, :2] > 0.0)
        assert same_bits(got[conv], want[conv]), np.abs(got[conv] - want[conv]).max()
    finally:
        s.close()


# ------------------------------------------------------------------ test 5
@pytest.fixture(scope="module")
def clean():
    s, sid = make_solver(20, 70)
    d = nlp_inputs(s, sid, 9)
    out = s.eval_kkt(d["X"], d["U"], d["PI"], d["LAM"], x0=d["x0"], yref=d["yref"], yref_e=d["yref_e"], parts=True, stages=True)
    yield s, d, out
    s.close()


BAD = (0, 33, 69)


@pytest.mark.parametrize("where,value", [("x", np.nan), ("u", np.nan), ("pi", np.nan), ("lam", np.nan), ("yref", np.nan),
                                         ("yref_e", np.nan), ("x0", np.nan), ("x", np.inf)])
def test_bad_lanes(clean, where, value):
    s, d, want = clean
    e = {k: v.copy() for k, v in d.items()}
    where = dict(x="X", u="U", pi="PI", lam="LAM").get(where, where)     # the point's keys (point_cases.nlp_point)
    # the first word of lane 0, one in the middle of lane 33, the last word of lane 69
    for lane, pos in zip(BAD, (0, e[where][0].size // 2, e[where][0].size - 1)):
        e[where][lane].reshape(-1)[pos] = value
    got = s.eval_kkt(e["X"], e["U"], e["PI"], e["LAM"], x0=e["x0"], yref=e["yref"], yref_e=e["yref_e"], parts=True, stages=True)
    good = np.setdiff1d(np.arange(s.B), BAD)
    for g, w in zip(got, want):
        assert np.all(np.isnan(g[list(BAD)])), (where, g[list(BAD)])
        assert same_bits(g[good], w[good])
        assert np.all(np.isfinite(w))


@pytest.mark.parametrize("where", ["g", "lam"])
def test_bad_lanes_qp(where):
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    N, nb = 20, 70
    q = mq.make_batch("Fall", N, nb, 1)
    rng = np.random.default_rng(11)
    point = {k: q[k] + 1e-3 * rng.uniform(-1, 1, q[k].shape) for k in ("dx", "du", "pi", "lam")}
    s = OcpSolver(N=N, batch=1)
    try:
        def run(q, point):
            data = [q[k].reshape(nb, N, -1) if k in ("A", "B") else q[k] for k in ("A", "B", "b", "H", "g", "lo", "hi", "dx0")]
            r = s.qp_residuals(*data, point["dx"], point["du"], point["pi"], point["lam"])
            return np.stack([r[k] for k in kkt_ref.QP_KEYS], 1)
        want = run(q, point)
        q2, p2 = {k: v.copy() for k, v in q.items()}, {k: v.copy() for k, v in point.items()}
        tgt = q2["g"] if where == "g" else p2["lam"]
        for lane, pos in zip(BAD, (0, tgt[0].size // 2, tgt[0].size - 1)):
            tgt[lane].reshape(-1)[pos] = np.nan
        got = run(q2, p2)
        good = np.setdiff1d(np.arange(nb), BAD)
        assert np.all(np.isnan(got[list(BAD)])) and np.all(np.isfinite(want))
        assert same_bits(got[good], want[good])
    finally:
        s.close()


# ------------------------------------------------------------------ test 6
def test_errors_and_lam():
    from uclv_qs_pushing_matlab_amd import _lib
    from uclv_qs_pushing_matlab_amd._lib import ptr
    from uclv_qs_pushing_matlab_amd.objects import make_shape
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    N, B = 20, 64
    z = lambda *sh: np.zeros(sh)
    # without shapes; with shapes but no references, given or staged
    s = OcpSolver(N=N, batch=B)
    with pytest.raises(_lib.QspError, match=ERR_STATE):
        s.eval_kkt(z(B, N + 1, 4), z(B, N, 2), z(B, N, 4), "implied", yref=z(B, N, 6), yref_e=z(B, 4))
    s.set_shapes([make_shape(n) for n in NAMES], shape_id=np.arange(B) % 4)
    with pytest.raises(_lib.QspError, match=ERR_STATE):
        s.eval_kkt(z(B, N + 1, 4), z(B, N, 2), z(B, N, 4), "implied")
    # null pointers
    L, h = s._L, s.handle
    X, U, PI, res = z(B, N + 1, 4), z(B, N, 2), z(B, N, 4), z(B, 4)
    yr, ye = z(B, N, 6), z(B, 4)
    for args in ((None, U, PI), (X, None, PI), (X, U, None)):
        assert L.qsp_eval_kkt(h, None, *[ptr(a) for a in args], None, ptr(yr), ptr(ye), ptr(res), None, None) == -1
    assert L.qsp_eval_kkt(h, None, ptr(X), ptr(U), ptr(PI), None, ptr(yr), ptr(ye), None, None, None) == -1
    assert L.qsp_eval_kkt(None, None, ptr(X), ptr(U), ptr(PI), None, ptr(yr), ptr(ye), ptr(res), None, None) == -1
    assert L.qsp_eval_kkt_device(h, None, None) == -1
    assert L.qsp_eval_kkt_device(h, C.byref(_lib.KktIO()), None) == -1
    assert L.qsp_get_lam(h, None) == -1
    q = mq.make_batch("F0", N, 2, 1)
    qa = [ptr(np.ascontiguousarray(q[k])) for k in ("A", "B", "b", "H", "g", "lo", "hi", "dx0", "dx", "du", "pi", "lam")]
    r6 = z(2, 6)
    assert L.qsp_qp_residuals(h, 2, *qa, ptr(r6)) == 0
    for i in range(len(qa)):
        assert L.qsp_qp_residuals(h, 2, *[None if j == i else a for j, a in enumerate(qa)], ptr(r6)) == -1
    assert L.qsp_qp_residuals(h, 2, *qa, None) == -1 and L.qsp_qp_residuals(h, 0, *qa, ptr(r6)) == -1
    # the RTI path keeps no bound multipliers
    with pytest.raises(_lib.QspError, match=ERR_STATE):
        s.get("lam")
    # ... and after solve() its answers have an optimality measure: finite, res_eq the recomputed defect
    sid = np.arange(B) % 4
    point_cases.cold_solve(s, 21)
    ok = s.get("status") == 0
    assert ok.sum() >= B // 2
    res = s.eval_kkt()
    assert np.all(np.isfinite(res[ok]))
    Xs, Us = s.get("x"), s.get("u")
    xn = s.eval_rk4(Xs[:, :N].reshape(-1, 4), Us.reshape(-1, 2), shape_id=np.repeat(sid, N))[0].reshape(B, N, 4)
    defect = np.abs(xn - Xs[:, 1:]).reshape(B, -1).max(1)
    scale = (np.abs(xn) + np.abs(Xs[:, 1:])).reshape(B, -1).max(1)
    print("RTI res_eq: worst ratio %.3f; median res over status-0 lanes: %s"
          % (kkt_ref.worst_ratio(res[ok, 1], defect[ok], scale[ok]), np.median(res[ok], 0)))
    assert within(res[ok, 1], defect[ok], scale[ok])
    assert same_bits(res, s.eval_kkt(Xs, Us, s.get("pi"), "implied"))
    s.close()
    # the merit SQP: no multipliers before a solve; then (B, N, 6), >= 0, and the defaults are the explicit call
    s = OcpSolver(N=N, batch=B, sqp_iters=30, nlp_solver_type="SQP")
    s.set_shapes([make_shape(n) for n in NAMES], shape_id=sid)
    with pytest.raises(_lib.QspError, match=ERR_STATE):
        s.get("lam")
    point_cases.cold_solve(s, 21)
    lam = s.get("lam")
    assert lam.shape == (B, N, 6) and np.all(lam >= 0.0) and lam.max() > 0.0
    assert s.get("lam", stage=3).shape == (B, 6)
    a = s.eval_kkt(parts=True, stages=True)
    b = s.eval_kkt(s.get("x"), s.get("u"), s.get("pi"), lam, parts=True, stages=True)
    assert all(same_bits(p, q_) for p, q_ in zip(a, b))
    s.close()
