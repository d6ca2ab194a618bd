"""The closed-loop lane walks under one exec mask each (riccati_solve<1, ...> in qsp_solver.hip).  The corrector's
difference walk and the two forward walks run all their steps in one region, lig <= L - 2: the terminal lanes are
disabled throughout, the chain's first lane is pinned, and a lane that already holds its final value is handed
the same bits again at every later step.  No arithmetic changed, so every output keeps its bits: each kernel
against the oracle's kernel-order twin, bit for bit.  The file pins behaviour, not the change: it passes on a
library with per-step masks as well.

All device work runs in three fresh child processes (this file run as a script).  Small batches take the fused
SQP loop by default, so every child sets QSP_FUSED_LOOP itself:
- 'compiled': QSP_FUSED_LOOP=0, the kernel compiled for N = 20 (fully unrolled walks, constant masks) and the
  runtime-horizon kernel at every other horizon;
- 'generic':  QSP_FUSED_LOOP=0 QSP_FIXED_HORIZON=0, the runtime-horizon kernel at N = 20 (rolled walks);
- 'fused':    QSP_FUSED_LOOP=1, sqp_loop_kernel.
The cases are the smallest shapes at which a walk that crossed an instance boundary, stepped once too few or
read a lane ahead of the wavefront would show:
- N = 20 (three instances of 21 lanes per wave, lane 63 padding with lig = 0) at B = 1, 2, 3, 4 and 7: one, two
  and three instances per wave, and a last wave with idle groups;
- N = 20, B = 7 with a NaN x0 (status 1) in lane 1 and an s_0 outside its bound (status 4) in lane 4: lane 1 is
  the middle instance of a wave with both neighbours healthy, and the healthy lanes keep the bits of the clean
  batch;
- N = 12, B = 5: L = 13, four instances per wave, instance boundaries inside DPP rows, twelve padding lanes;
- N = 31, B = 3: L = 32, lanes 32 .. 63 padding with lig = 0 .. 31;
- N = 10, B = 7: the lane-walk factorisation in front of the walks, five instances per wave;
- the merit SQP at N = 20, B = 7 (its own kernels, runtime horizon);
- N = 50, B = 3: two stages per lane (scans, no lane walk), a kernel that did not change, as a guard.
Four shapes mixed by lane, three SQP iterations, two controller steps (cold, then warm-started with wave
packing).  Tolerance: none.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("santal", "balea", "montana", "pulirapid")
OUT_KEYS = ("u0", "X", "U", "PI", "status", "cost", "qp_iter")
K = 3
BAD = {1: ("x", float("nan")), 4: ("s", 0.05)}   # lane -> (x0 component, value); bad_lanes.py: x0_x_nan, x0_s_out
BAD_STATUS = {1: 1, 4: 4}

# name -> (N, B, merit, bad lanes)
CASES = {f"n20-b{b}": (20, b, False, False) for b in (1, 2, 3, 4, 7)}
CASES["n20-b7-bad"] = (20, 7, False, True)
CASES["n12-b5"] = (12, 5, False, False)
CASES["n31-b3"] = (31, 3, False, False)
CASES["n10-b7"] = (10, 7, False, False)
CASES["n20-b7-merit"] = (20, 7, True, False)
CASES["n50-b3"] = (50, 3, False, False)
# (stages per lane, lanes per instance, factorisation) the library must report for the case to test what it names
KERNEL = {12: (1, 13, "matrix cores"), 20: (1, 21, "matrix cores"), 31: (1, 32, "matrix cores"),
          10: (1, 11, "lane walk"), 50: (2, 26, "matrix cores")}
# child -> (QSP_FUSED_LOOP, QSP_FIXED_HORIZON or None)
CHILDREN = {"compiled": ("0", None), "generic": ("0", "0"), "fused": ("1", None)}


def child_runs(tag, case):
    """Which cases a child runs: 'generic' the N = 20 ones (the others take the runtime horizon anyway), and
    the merit SQP, which has no fused loop, not in 'fused'."""
    N, _, merit, _ = CASES[case]
    return not (tag == "generic" and N != 20) and not (tag == "fused" and merit)


def inputs(N, B, bad):
    sys.path.insert(0, ROOT)
    from bench import SEED, make_inputs
    x0, _, _, sid, traj = make_inputs(B, N, SEED + N)
    x0 = x0.copy()
    if bad:
        for lane, (comp, val) in BAD.items():
            x0[lane, "xyts".index(comp)] = val
    return x0, sid, traj


# ------------------------------------------------------------------ the child: device runs only
def child(tag, out_path):
    sys.path.insert(0, ROOT)
    from uclv_qs_pushing_matlab_amd.objects import make_shape
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    out = {}
    for name, (N, B, merit, bad) in CASES.items():
        if not child_runs(tag, name):
            continue
        x0, sid, traj = inputs(N, B, bad)
        s = OcpSolver(N=N, batch=B, sqp_iters=K, **(dict(nlp_solver_type="SQP") if merit else {}))
        try:
            s.set_shapes([make_shape(n) for n in NAMES], shape_id=sid)
            s.set_reference_trajectory(traj)
            out[f"{name}/fixed_horizon"] = np.int32(s.fixed_horizon())
            out[f"{name}/layout"] = np.array(s.layout(), np.int32)
            out[f"{name}/factor_walk"] = np.array(s.factor_walk())
            for step in range(2):
                r = dict(u0=s.controller_solve(x0, 1 + step), X=s.get("x"), U=s.get("u"), PI=s.get("pi"),
                         status=s.get("status"), cost=s.get_cost(), qp_iter=s.get("qp_iter"))
                for k in OUT_KEYS:
                    out[f"{name}/{step}/{k}"] = r[k]
        finally:
            s.close()
    np.savez(out_path, **out)


# ------------------------------------------------------------------ the twin's references, once
_REF = {}


def reference(N, B, merit, bad):
    key = (N, B, merit, bad)
    if key in _REF:
        return _REF[key]
    from oracle.oracle import Oracle, make_opts
    twin = Oracle(NAMES, twin=True)
    x0, sid, traj = inputs(N, B, bad)
    assert len(np.unique(sid)) == min(B, 4), "the batch mixes the shapes"
    op = make_opts(N=N, sqp_iters=K, **(dict(nlp_mode=1) if merit else {}))
    warm = twin.new_warm(B, N)
    steps = []
    for step in range(2):
        r = twin.controller_solve(op, x0, traj, 1 + step, warm, shape_id=sid)
        r.update(X=warm["X"].copy(), U=warm["U"].copy(), PI=warm["PI"].copy())
        steps.append(r)
    _REF[key] = steps
    return steps


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Outputs of the cases from three fresh processes (CHILDREN), each with QSP_FUSED_LOOP set."""
    d = tmp_path_factory.mktemp("walk_regions")
    res = {}
    for tag, (fused, fixed) in CHILDREN.items():
        env = dict(os.environ)
        env.pop("QSP_FIXED_HORIZON", None)
        env["QSP_FUSED_LOOP"] = fused
        if fixed is not None:
            env["QSP_FIXED_HORIZON"] = fixed
        out = d / f"{tag}.npz"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), tag, str(out)], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, f"{tag} child failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        with np.load(out) as z:
            res[tag] = {k: z[k] for k in z.files}
    return res


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    eq = (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else (a == b)
    if not eq.all():
        bad = np.argwhere(~eq)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {a.size} entries differ; first at {i}: gpu {a[i]!r} twin {b[i]!r}")


@pytest.mark.parametrize("case", list(CASES))
def test_equals_twin(runs, case):
    N, B, merit, bad = CASES[case]
    tags = [tag for tag in CHILDREN if child_runs(tag, case)]
    assert "compiled" in tags
    for step, r in enumerate(reference(N, B, merit, bad)):
        for tag in tags:
            for k in OUT_KEYS:
                same(runs[tag][f"{case}/{step}/{k}"], r[k], f"{tag} {case} step {step} {k}")


def test_bad_lanes_keep_their_status_and_their_neighbours_their_bits(runs):
    """Lane 1 (NaN x0), the middle instance of the first wave, ends with status 1, lane 4 (s_0 outside its bound:
    no QP is feasible) with status 4, and the five healthy lanes around them hold the bits they have in the clean
    batch, which solves: no NaN moved from an instance into its neighbours through a walk."""
    from bad_lanes import healthy_equal
    mask = np.zeros(7, bool)
    mask[list(BAD)] = True
    for tag in CHILDREN:
        for step in range(2):
            st = runs[tag][f"n20-b7-bad/{step}/status"]
            clean = runs[tag][f"n20-b7/{step}/status"]
            assert np.all(clean == 0), (tag, step, clean)
            assert {lane: int(st[lane]) for lane in BAD} == BAD_STATUS, (tag, step, st)
            for k in OUT_KEYS:
                healthy_equal(runs[tag][f"n20-b7-bad/{step}/{k}"], runs[tag][f"n20-b7/{step}/{k}"], mask,
                              f"{tag} step {step} {k}")


def test_cases_run_the_kernels_they_name(runs):
    """The handle compiles its per-iteration launches for N = 20 and for no other horizon, and never under the
    switch; every horizon has the stages per lane, the lanes per instance and the factorisation its case is there
    for.  Without this the comparisons could pass on one kernel twice.  (The merit SQP has its own kernels,
    instantiated for a runtime horizon only; the handle's getter answers for the fixed-K launches, so it is not
    asked there.  The fused loop has a runtime horizon too: in 'fused' the getter says what the handle would
    launch per iteration.)"""
    for tag in CHILDREN:
        for case, (N, _, merit, _) in CASES.items():
            if not child_runs(tag, case):
                continue
            S, L, walk = KERNEL[N]
            assert tuple(runs[tag][f"{case}/layout"]) == (S, L), (tag, case)
            assert str(runs[tag][f"{case}/factor_walk"]).startswith(walk), (tag, case)
            if not merit:
                want = 20 if (N == 20 and tag != "generic") else 0
                assert int(runs[tag][f"{case}/fixed_horizon"]) == want, (tag, case)


if __name__ == "__main__":
    child(sys.argv[1], sys.argv[2])
