"""The compiled kernel's lane tests as constant masks (lane_mask_* in qsp_layout.h, taken through
lanes_of in qsp_solver.hip).  The kernel compiled for N = 20 takes which lanes pass `lig <= j`,
`j <= lig < L - 1`, `lig + off < L`, `lig < N`, the GroupScan flags and the factor walk's publish / collect
regions from 64-bit constants; the runtime-horizon kernel compares per lane as before.  No arithmetic changed,
so every output keeps its bits: the compiled kernel against the runtime-horizon kernel (QSP_FIXED_HORIZON=0)
byte for byte, and both against the oracle's kernel-order twin bit for bit.

All device work runs in two fresh child processes (this file run as a script).  What could break, and the case
that shows it:
- a mask wrong on the lanes of a wave's second or third instance, on the padding lane 63, or wrong only where
  the last wave is partly filled: N = 20 (three instances of 21 lanes per wave) at B = 1, 2, 3 (one wave with
  one, two, three instances), 4 and 7 (a full wave and one instance in the last), 64 (21 full waves and one
  instance);
- a constant region that lets a lane read a slot it no longer writes: the same runs with QSP_DEBUG_POISON=1
  (LDS filled with NaN patterns before the solve), byte-identical to the unpoisoned run;
- the status rule and lane isolation under the new regions: B = 7 with an s_0 outside its bound (every QP
  infeasible: status 4) in lane 1 and a NaN x0 (status 1) in lane 4, the healthy lanes bit-identical to the
  clean batch;
- the kernels that keep the per-lane tests: the merit SQP (runtime horizon at N = 20) and N = 31.
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
BATCHES = (1, 2, 3, 4, 7, 64)
BAD = {1: ("s", 0.05), 4: ("x", float("nan"))}   # lane -> (x0 component, value); bad_lanes.py: x0_s_out, x0_x_nan
BAD_STATUS = {1: 4, 4: 1}

# name -> (N, B, merit, QSP_DEBUG_POISON, bad lanes)
CASES = {}
for _b in BATCHES:
    CASES[f"n20-b{_b}"] = (20, _b, False, "0", False)
    CASES[f"n20-b{_b}-poison"] = (20, _b, False, "1", False)
CASES["n20-b7-bad"] = (20, 7, False, "0", True)
CASES["n20-b7-merit"] = (20, 7, True, "0", False)
CASES["n31-b3"] = (31, 3, False, "0", False)
N20 = [c for c, v in CASES.items() if v[0] == 20]
POISON = {c: c[:-len("-poison")] for c in CASES if c.endswith("-poison")}


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
    for name, (N, B, merit, poison, bad) in CASES.items():
        if mode == "generic" and N != 20:
            continue
        os.environ["QSP_DEBUG_POISON"] = poison
        x0, sid, traj = inputs(N, B, bad)
        s = OcpSolver(N=N, batch=B, sqp_iters=K, **(dict(nlp_solver_type="SQP") if merit else {}))
        try:
            s.set_shapes([make_shape(n) for n in NAMES], shape_id=sid)
            s.set_reference_trajectory(traj)
            out[f"{name}/fixed_horizon"] = np.int32(s.fixed_horizon())
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
    d = tmp_path_factory.mktemp("lane_masks")
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


@pytest.mark.parametrize("case", [c for c in CASES if c not in POISON])
def test_equals_twin(runs, case):
    N, B, merit, _, bad = CASES[case]
    tags = ("default", "generic") if N == 20 else ("default",)
    for step, r in enumerate(reference(N, B, merit, bad)):
        for tag in tags:
            for k in OUT_KEYS:
                same(runs[tag][f"{case}/{step}/{k}"], r[k], f"{tag} {case} step {step} {k}")


@pytest.mark.parametrize("case", N20)
def test_compiled_equals_generic(runs, case):
    for step in range(2):
        for k in OUT_KEYS:
            same_bytes(runs["default"][f"{case}/{step}/{k}"], runs["generic"][f"{case}/{step}/{k}"], f"{case} step {step} {k}")


@pytest.mark.parametrize("case", list(POISON))
def test_poisoned_lds_equals_unpoisoned(runs, case):
    for tag in ("default", "generic"):
        for step in range(2):
            for k in OUT_KEYS:
                same_bytes(runs[tag][f"{case}/{step}/{k}"], runs[tag][f"{POISON[case]}/{step}/{k}"],
                           f"{tag} {case} step {step} {k}")


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
    """The compiled kernel runs the fixed-K N = 20 cases and nothing else, and never under the switch: without
    this the comparisons could pass on one kernel twice.  (The merit SQP has its own kernels, instantiated for
    a runtime horizon only; the handle's getter answers for the fixed-K launches, so it is not asked there.)"""
    for case, (N, _, merit, _, _) in CASES.items():
        if not merit:
            assert int(runs["default"][f"{case}/fixed_horizon"]) == (20 if N == 20 else 0), case
        if N == 20:
            assert int(runs["generic"][f"{case}/fixed_horizon"]) == 0, case


if __name__ == "__main__":
    child(sys.argv[1], sys.argv[2])
