"""qp_step_kernel compiled for its horizon (qsp_solver.hip: QSP_FIXED_HORIZONS, ctx_of<S, NC>, launch_qp_any).
At N = 20 the one-stage matrix-core QP kernel is launched with the horizon as a compile-time constant; every
other horizon, variant and kernel takes the runtime-horizon code, and QSP_FIXED_HORIZON=0 forces that code at
N = 20 too.  Only bookkeeping differs between the two, so every output must be the same bytes from both and
equal the oracle's kernel-order twin bit for bit, on all lanes.

All device work runs in two fresh child processes (this file run as a script), one per setting of the switch;
each runs every case once and saves its outputs, which the tests then compare: specialised against generic
byte for byte, and both against the twin.  What could break, and the case that shows it:
- a constant that does not equal the runtime value it replaces (L, G, the phase split, the record stride, the
  IPM's m, the walks' bounds): B = 385 is 128 full waves and one with a single real instance, four shapes
  mixed, K = 6, two controller steps (the warm one with wave packing and unequal IPM counts in a wave);
- the exits: qp_iters = 3 (every QP at the cap), qp_mu_max = 1.2 (diverged QPs, status 4);
- the fused loop (QSP_FUSED_LOOP=1), which is not specialised and must still agree; one and two stream parts;
- the QP-level entry (the kernel without the linearisation) on tests/qp_data.py's QPs at the twin's iterate;
- the dispatch catching a neighbour, or nothing: N = 19 and N = 21 (K = 3) stay bit-identical to the twin, and
  qsp_get_fixed_horizon reports 20 at N = 20 only, 0 at its neighbours and under the switch;
- a record field read before it is written: QSP_DEBUG_POISON=1 on the specialised kernel, identical to the
  unpoisoned run.
The guards on the inputs are asserted on the twin's own output, on the CPU.  Tolerance: none.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("santal", "balea", "montana", "pulirapid")
B = 385
EXITS = {"default": {}, "cap3": dict(qp_iters=3), "mumax": dict(qp_mu_max=1.2)}
G_OF = {19: 3, 20: 3, 21: 2}   # instances per wave
OUT_KEYS = ("u0", "X", "U", "PI", "status", "cost", "qp_iter")
QP_KEYS = ("dx", "du", "pi", "lam", "iters", "qp_status")

# name -> (N, K, exit, QSP_FUSED_LOOP, stream parts, QSP_DEBUG_POISON)
CASES = {}
for _e in EXITS:
    for _f in ("0", "1"):
        CASES[f"{_e}-fused{_f}-parts1"] = (20, 6, _e, _f, 1, "0")
    CASES[f"{_e}-fused0-parts2"] = (20, 6, _e, "0", 2, "0")
CASES["default-fused0-parts1-poison"] = (20, 6, "default", "0", 1, "1")
CASES["n19"] = (19, 3, "default", "0", 1, "0")
CASES["n21"] = (21, 3, "default", "0", 1, "0")


def inputs():
    rng = np.random.default_rng(7)
    x0 = np.stack([rng.uniform(-0.02, 0.04, B), rng.uniform(-0.04, 0.03, B),
                   np.deg2rad(rng.uniform(-25.0, 25.0, B)), rng.uniform(-0.058, 0.0105, B)], 1)
    return x0, (np.arange(B) % 4).astype(np.int32)


def straight_traj(T_end=10.0, Ts=0.05, v=0.01):
    t = np.arange(0.0, T_end + 1e-9, Ts)
    traj = np.zeros((len(t), 6))
    traj[:, 0] = v * t
    return traj


# ------------------------------------------------------------------ the child: device runs only
def child(inp_path, out_path):
    sys.path.insert(0, ROOT)
    from uclv_qs_pushing_matlab_amd.objects import make_shape
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    inp = np.load(inp_path)
    x0, sid = inputs()
    traj = straight_traj()
    out = {}
    for name, (N, K, exit_, fused, parts, poison) in CASES.items():
        os.environ["QSP_FUSED_LOOP"] = fused
        os.environ["QSP_DEBUG_POISON"] = poison
        s = OcpSolver(N=N, batch=B, sqp_iters=K, **EXITS[exit_])
        try:
            s.set_shapes([make_shape(n) for n in NAMES])
            s.set_shape_ids(sid)
            s.set_stream_parts(parts)
            assert tuple(s.layout()) == (1, N + 1)
            s.set_reference_trajectory(traj)
            out[f"{name}/fixed_horizon"] = np.int32(s.fixed_horizon())
            for step in range(2):
                r = dict(u0=s.controller_solve(x0, 1 + step), X=s.get("x"), U=s.get("u"), PI=s.get("pi"),
                         status=s.get("status"), cost=s.get_cost(), qp_iter=s.get("qp_iter"))
                for k in OUT_KEYS:
                    out[f"{name}/{step}/{k}"] = r[k]
        finally:
            s.close()
    # the QP-level entry: qp_step_kernel without the linearisation
    os.environ["QSP_FUSED_LOOP"] = "0"
    os.environ["QSP_DEBUG_POISON"] = "0"
    s = OcpSolver(N=20, batch=B, sqp_iters=1)
    try:
        s.set_shapes([make_shape(n) for n in NAMES])
        s.set_shape_ids(sid)
        out["qp/fixed_horizon"] = np.int32(s.fixed_horizon())
        r = s.qp_solve(*[inp[f"qp_{k}"] for k in ("A", "B", "b", "H", "g", "lo", "hi", "dx0")])
        for k in QP_KEYS:
            out[f"qp/{k}"] = r[k]
    finally:
        s.close()
    np.savez(out_path, **out)


# ------------------------------------------------------------------ the twin's references, once
_REF = {}


def reference(N, K, exit_):
    """The twin's two controller steps (cold, then warm-started from the shifted solution), with the guards
    on the inputs: a lane with status 4 in the cold step of a qp_mu_max case, every QP at the cap in a
    qp_iters = 3 case, and in every other case a wave with unequal IPM counts in the warm step's first SQP
    iteration (packed in lane order like every solve's first)."""
    key = (N, K, exit_)
    if key in _REF:
        return _REF[key]
    from oracle.oracle import Oracle, make_opts
    twin = Oracle(NAMES, twin=True)
    kw = EXITS[exit_]
    traj = straight_traj()
    x0, sid = inputs()
    op = make_opts(N=N, sqp_iters=K, **kw)
    op1 = make_opts(N=N, sqp_iters=1, **kw)
    warm = twin.new_warm(B, N)
    steps, first = [], []
    for step in range(2):
        w1 = {k: v.copy() for k, v in warm.items()}
        first.append(twin.controller_solve(op1, x0, traj, 1 + step, w1, shape_id=sid)["qp_iter"])
        r = twin.controller_solve(op, x0, traj, 1 + step, warm, shape_id=sid)
        r.update(X=warm["X"].copy(), U=warm["U"].copy(), PI=warm["PI"].copy())
        steps.append(r)
    if exit_ == "mumax":
        assert (steps[0]["status"] == 4).sum() >= 1, f"N = {N}: no lane with status 4 in the cold step"
    if exit_ == "cap3":
        for r in steps:
            assert np.all(r["qp_iter"] == 3 * K), f"N = {N}: QPs below the cap"
    else:
        G = G_OF[N]
        q = first[1][:B // G * G].reshape(-1, G)
        assert np.any(q.min(1) != q.max(1)), f"N = {N}: every wave's instances take the same IPM count"
    _REF[key] = steps
    return steps


def qp_reference():
    """tests/qp_data.py's QPs at the twin's iterate after the cold controller step (N = 20), and the twin's
    solutions of them."""
    if "qp" in _REF:
        return _REF["qp"]
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from qp_data import build_qp
    from oracle.oracle import Oracle, make_opts
    twin = Oracle(NAMES, twin=True)
    N = 20
    r = reference(N, 6, "default")[0]
    x0, sid = inputs()
    traj = straight_traj()
    yref = np.repeat(traj[None, 1:1 + N], B, 0)
    yref_e = yref[:, N - 1, :4].copy()
    op = make_opts(N=N)
    A, Bm, b, H, g, lo, hi, act, dx0 = build_qp(twin, op, r["X"], r["U"], yref, yref_e, x0, sid)
    data = dict(A=A, B=Bm, b=b, H=H, g=g, lo=lo, hi=hi, dx0=dx0)
    sol = twin.qp(op, A, Bm, b, H, g, lo, hi, act, dx0)
    assert np.mean(sol["qp_status"] == 0) > 0.9 and sol["iters"].min() != sol["iters"].max(), "the QPs' IPM counts"
    _REF["qp"] = (data, sol)
    return _REF["qp"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Outputs of every case from two fresh processes: 'fixed' with the library's own dispatch, 'generic'
    with QSP_FIXED_HORIZON=0."""
    d = tmp_path_factory.mktemp("fixed_horizon")
    data, _ = qp_reference()
    inp = d / "inputs.npz"
    np.savez(inp, **{f"qp_{k}": v for k, v in data.items()})
    res = {}
    for tag, switch in (("fixed", None), ("generic", "0")):
        env = dict(os.environ)
        env.pop("QSP_FIXED_HORIZON", None)
        if switch is not None:
            env["QSP_FIXED_HORIZON"] = switch
        out = d / f"{tag}.npz"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), str(inp), str(out)], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, f"{tag} child failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        with np.load(out) as z:
            res[tag] = {k: z[k] for k in z.files}
    return res


def same_bytes(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.tobytes() != b.tobytes():
        bad = np.flatnonzero(a.view(np.uint8).reshape(-1) != b.view(np.uint8).reshape(-1)) // a.itemsize
        i = np.unravel_index(int(bad[0]), a.shape)
        raise AssertionError(f"{what}: bytes differ at {len(np.unique(bad))} of {a.size} entries; first at {i}: "
                             f"{a[i]!r} against {b[i]!r}")


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    eq = (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else (a == b)
    if not eq.all():
        bad = np.argwhere(~eq)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {a.size} entries differ; first at {i}: gpu {a[i]!r} twin {b[i]!r}")


@pytest.mark.parametrize("case", list(CASES))
def test_specialised_equals_generic(runs, case):
    for step in range(2):
        for k in OUT_KEYS:
            same_bytes(runs["fixed"][f"{case}/{step}/{k}"], runs["generic"][f"{case}/{step}/{k}"], f"{case} step {step} {k}")


@pytest.mark.parametrize("tag", ["fixed", "generic"])
@pytest.mark.parametrize("case", list(CASES))
def test_equals_twin(runs, case, tag):
    N, K, exit_ = CASES[case][:3]
    for step, r in enumerate(reference(N, K, exit_)):
        for k in OUT_KEYS:
            same(runs[tag][f"{case}/{step}/{k}"], r[k], f"{tag} {case} step {step} {k}")


def test_dispatch_reports_the_compiled_horizon(runs):
    """qsp_get_fixed_horizon, the launchers' own rule: the compiled kernel at N = 20 only, never under the
    switch.  Without this every other case would pass with a dispatch that never took the compiled kernel."""
    for case, (N, *_) in CASES.items():
        assert int(runs["fixed"][f"{case}/fixed_horizon"]) == (20 if N == 20 else 0), case
        assert int(runs["generic"][f"{case}/fixed_horizon"]) == 0, case
    assert int(runs["fixed"]["qp/fixed_horizon"]) == 20 and int(runs["generic"]["qp/fixed_horizon"]) == 0


def test_poisoned_lds_equals_unpoisoned(runs):
    for step in range(2):
        for k in OUT_KEYS:
            same_bytes(runs["fixed"][f"default-fused0-parts1-poison/{step}/{k}"],
                       runs["fixed"][f"default-fused0-parts1/{step}/{k}"], f"poisoned step {step} {k}")


def test_qp_entry(runs):
    _, sol = qp_reference()
    for k in QP_KEYS:
        same_bytes(runs["fixed"][f"qp/{k}"], runs["generic"][f"qp/{k}"], f"QP entry {k}")
        same(runs["fixed"][f"qp/{k}"], sol[k], f"QP entry against the twin, {k}")


if __name__ == "__main__":
    child(sys.argv[1], sys.argv[2])
