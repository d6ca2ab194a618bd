"""CPU: the Python layer of the sensitivity entries (no library call), and the CPU side of
tests/test_gpu_sens.py::test_difference_quotients_of_qp_solve -- the kernel-order twin's own difference
quotients against the dense sensitivity of tests/sens_ref.py, which is where that test's bound comes from."""
import ctypes as C
import re

import numpy as np
import pytest

import manufactured_qp as mq
import sens_ref
from conftest import ROOT

NEW = ("qsp_default_sens_opts", "qsp_eval_sens", "qsp_eval_sens_device", "qsp_get_sens", "qsp_qp_sens")


def test_prototypes_are_in_the_table():
    from uclv_qs_pushing_matlab_amd import _lib
    for name in NEW:
        assert name in _lib._SIGS and name in _lib.EXPORTED, name
    assert "qsp_default_sens_opts" in _lib._VOID
    # as many argument types as the header declares parameters
    hdr = open(ROOT + "/include/qsp_nmpc.h").read()
    for name in NEW:
        m = re.search(r"\b%s\(([^;]*?)\);" % name, hdr, re.S)
        assert m, name
        params = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
        assert len(params) == len(_lib._SIGS[name]), (name, params)
    assert C.sizeof(_lib.SensOpts) == 16 and C.sizeof(_lib.SensIO) == 12 * C.sizeof(C.c_void_p)
    assert [f[0] for f in _lib.SensIO._fields_][-5:] == list(_lib.SENS_OUTPUTS)
    assert _lib.ABI_VERSION == 9


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("library call " + name)


def test_want_rejects_unknown_names_without_a_library_call():
    from uclv_qs_pushing_matlab_amd.controller import NMPCController
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    s = OcpSolver.__new__(OcpSolver)      # no handle: nothing below may reach the library
    s._L, s._h, s.B, s.N = _NoLibrary(), None, 2, 3
    X, U = np.zeros((2, 4, 4)), np.zeros((2, 3, 2))
    for want in (("K0", "gain"), "dK", ("K0", "K", "du")):
        with pytest.raises(ValueError, match="want"):
            s.eval_sens(X, U, want=want)
        with pytest.raises(ValueError, match="want"):
            s.get_sens(want=want)
        with pytest.raises(ValueError, match="want"):
            s.qp_sens(np.zeros((1, 3, 16)), np.zeros((1, 3, 8)), np.zeros((1, 22)), want=want)
    assert OcpSolver._sens_want("K0") == ("K0",) and OcpSolver._sens_want(("dU", "flag")) == ("dU", "flag")
    out = OcpSolver._sens_outputs(("P0", "flag"), 2, 3)
    assert set(out) == {"K0", "P0", "flag"} and out["flag"].dtype == np.int32 and out["P0"].shape == (2, 10)
    assert callable(NMPCController.feedback_gain)
    del s._h                               # (so that __del__ has nothing to close)


def test_the_twins_quotients_against_the_dense_sensitivity():
    """The figure the GPU test's bound is four times of: central difference quotients (delta = 1e-6) of the twin's
    QP solve on the Fu batch of sens_ref.QUOT against the dense sensitivity with d = lam / slack of the twin's own
    answer.  Measured 7.030e-8 (the literal restatement: 7.029e-8) at sensitivities up to 1.96; no QP of the 16 is
    left out for a changed active set (the seed's check: at most 2 may be)."""
    from oracle.oracle import Oracle, make_opts
    c = sens_ref.QUOT
    q = mq.make_batch(c["family"], c["N"], c["nb"], c["seed"])
    op = make_opts(N=c["N"], qp_iters=mq.QP_ITERS, stage0_s_bound=0)
    tw = Oracle(twin=True)
    Q, H, keep = sens_ref.quotient_check(lambda dx0: tw.qp(op, *mq.qp_args(dict(q, dx0=dx0))), q, c["delta"])
    ref = sens_ref.sens(q["A"], q["B"], H)
    err = np.abs(Q - ref["dU"]).reshape(c["nb"], -1).max(1)
    print("kept %d of %d; worst |quotient - dense| %.3e; max |dU| %.2f" % (keep.sum(), c["nb"], err[keep].max(), np.abs(ref["dU"]).max()))
    assert keep.sum() >= c["nb"] - c["max_left_out"]
    assert 0.5 * c["twin_err"] <= err[keep].max() <= c["twin_err"]      # the recorded figure is the measured one
    assert np.abs(ref["dU"]).max() > 1.0                                # ... of sensitivities of order one
