"""Lane tests marked as never empty (QSP_SOME_LANE in qsp_solver.hip).  Where some lane of every wave passes a
lane test -- by the wave's geometry or the enclosing loop's exit condition -- the kernels tell the compiler so,
and it drops the branch that would skip the region for a wave with no lane in it.  The region then also runs in
a wave whose lanes all fail the test, under an empty exec mask, where it must do nothing.  No arithmetic
changed, so every output keeps its bits: each kernel against the oracle's kernel-order twin, bit for bit.

All device work runs in two fresh child processes (this file run as a script), one of them with
QSP_FIXED_HORIZON=0.  The cases are the smallest shapes at which a hinted mask is most sparse, or at which a
kernel other than the headline's takes the hint:
- N = 20 (three instances of 21 lanes per wave, lane 63 padding) at B = 1, 2, 3, 4 and 7: a wave holds one or
  two instances, with whole groups of lanes that have none; compiled kernel (the three lane walks' steps) and,
  under the switch, the runtime-horizon kernel (per-lane tests in rolled walks, publish and collect);
- N = 12: four instances per wave, the matrix-core walk with one instance per block; B = 5 leaves the last
  wave one instance;
- N = 31: one instance per wave and 32 padding lanes;
- N = 10: the lane-walk factorisation (`lig <= j` down to step 0, where only each group's first lane enters);
- N = 50 at B = 3: two stages per lane (the slot tests `kb <= k <= ke` of both phases, the scans' `take`);
- the merit SQP at N = 20, B = 7 (its own kernels, runtime horizon);
- B = 7 with an s_0 outside its bound (status 4) in lane 1 and a NaN x0 (status 1) in lane 4: one instance of
  a wave is frozen while the others iterate, and the healthy lanes keep the bits of the clean batch.
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
BAD = {1: ("s", 0.05), 4: ("x", float("nan"))}   # lane -> (x0 component, value); bad_lanes.py: x0_s_out, x0_x_nan
BAD_STATUS = {1: 4, 4: 1}

# name -> (N, B, merit, bad lanes)
CASES = {f"n20-b{b}": (20, b, False, False) for b in (1, 2, 3, 4, 7)}
CASES["n20-b7-bad"] = (20, 7, False, True)
CASES["n20-b7-merit"] = (20, 7, True, False)
CASES["n12-b5"] = (12, 5, False, False)
CASES["n31-b3"] = (31, 3, False, False)
CASES["n10-b7"] = (10, 7, False, False)
CASES["n50-b3"] = (50, 3, False, False)
# (stages per lane, lanes per instance, factorisation) the library must report for the case to test what it names
KERNEL = {12: (1, 13, "matrix cores"), 20: (1, 21, "matrix cores"), 31: (1, 32, "matrix cores"),
          10: (1, 11, "lane walk"), 50: (2, 26, "matrix cores")}


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
def child(mode, out_path):
    sys.path.insert(0, ROOT)
    from uclv_qs_pushing_matlab_amd.objects import make_shape
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    out = {}
    for name, (N, B, merit, bad) in CASES.items():
        if mode == "generic" and N != 20:
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
    """Outputs of every case from two fresh processes: 'default' with the library's own dispatch (all cases),
    'generic' with QSP_FIXED_HORIZON=0 (the N = 20 cases)."""
    d = tmp_path_factory.mktemp("skip_branches")
    res = {}
    for tag, switch in (("default", None), ("generic", "0")):
        env = dict(os.environ)
        env.pop("QSP_FIXED_HORIZON", None)
        if switch is not None:
            env["QSP_FIXED_HORIZON"] = switch
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
    tags = ("default", "generic") if N == 20 else ("default",)
    for step, r in enumerate(reference(N, B, merit, bad)):
        for tag in tags:
            for k in OUT_KEYS:
                same(runs[tag][f"{case}/{step}/{k}"], r[k], f"{tag} {case} step {step} {k}")


def test_bad_lanes_keep_their_status_and_their_neighbours_their_bits(runs):
    """Lane 1 (s_0 outside its bound: no QP is feasible) ends with status 4, lane 4 (NaN x0) with status 1, and
    the five healthy lanes around them hold the bits they have in the clean batch, which solves."""
    from bad_lanes import healthy_equal
    mask = np.zeros(7, bool)
    mask[list(BAD)] = True
    for tag in ("default", "generic"):
        for step in range(2):
            st = runs[tag][f"n20-b7-bad/{step}/status"]
            clean = runs[tag][f"n20-b7/{step}/status"]
            assert np.all(clean == 0), (tag, step, clean)
            assert {lane: int(st[lane]) for lane in BAD} == BAD_STATUS, (tag, step, st)
            for k in OUT_KEYS:
                healthy_equal(runs[tag][f"n20-b7-bad/{step}/{k}"], runs[tag][f"n20-b7/{step}/{k}"], mask,
                              f"{tag} step {step} {k}")


def test_cases_run_the_kernels_they_name(runs):
    """The compiled kernel runs the fixed-K N = 20 cases and nothing else, and never under the switch; every
    horizon has the stages per lane, the lanes per instance and the factorisation its case is there for.
    Without this the comparisons could pass on one kernel twice.  (The merit SQP has its own kernels,
    instantiated for a runtime horizon only; the handle's getter answers for the fixed-K launches, so it is
    not asked there.)"""
    for case, (N, _, merit, _) in CASES.items():
        S, L, walk = KERNEL[N]
        assert tuple(runs["default"][f"{case}/layout"]) == (S, L), case
        assert str(runs["default"][f"{case}/factor_walk"]).startswith(walk), case
        if not merit:
            assert int(runs["default"][f"{case}/fixed_horizon"]) == (20 if N == 20 else 0), case
        if N == 20:
            assert int(runs["generic"][f"{case}/fixed_horizon"]) == 0, case


if __name__ == "__main__":
    child(sys.argv[1], sys.argv[2])
