"""The matrix-core factor walk's step stores on the whole wave (factor_walk_mfma in qsp_solver.hip; mfw_store_k,
mfw_store_z in qsp_layout.h).  At one stage per lane every block lane stores its element of K and of Z at every
step, without a lane test: rows 0, 1 to the record's output slots, rows 2, 3 to dump slots among the record's
dead operand slots, and the lanes of a block beyond the wave's instances to the addresses of the block they
repeat (two stages per lane share the function and keep the lane test).  Only where a lane stores changed, so
every output must keep its bits: equal to the oracle's kernel-order twin bit for bit on all
lanes, and at N = 20 the same bytes from the kernel compiled for the horizon and from the runtime-horizon kernel
(QSP_FIXED_HORIZON=0).

All device work runs in two fresh child processes (this file run as a script), which run every case once and
save the outputs.  What could break, and the case that shows it:
- a dump slot that is still live, or a duplicate block storing something else than the block it repeats:
  three instances per wave (N = 20, B = 385 = 128 full waves and one with a single instance, four shapes, K = 6,
  block 3 repeats instance 2), four (N = 12, B = 130, no duplicate block), two (N = 31, B = 65, blocks 2 and 3
  both repeat instance 1, so a pair of lanes stores to one address), the compiled horizon's neighbours N = 19
  and 21, and factor_walk_mfma<2> (N = 50, two stages per lane, B = 33);
- a collect, or a later field, that reads a dump slot: QSP_DEBUG_POISON=1 at N = 20, 31 and 50, byte-identical to
  the unpoisoned run;
- the exit right after a walk: qp_iters = 3, every QP at the cap;
- the launch paths: one and two stream parts, QSP_FUSED_LOOP 0 and 1.
Two controller steps per case (cold, then warm-started with wave packing).  Tolerance: none.
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
MFMA = "matrix cores (v_mfma_f64_4x4x4_4b_f64)"

# name -> (N, B, K, solver options, QSP_FUSED_LOOP, stream parts, QSP_DEBUG_POISON)
CASES = {
    "n20": (20, 385, 6, {}, "0", 1, "0"),
    "n20-fused1": (20, 385, 6, {}, "1", 1, "0"),
    "n20-parts2": (20, 385, 6, {}, "0", 2, "0"),
    "n20-cap3": (20, 385, 6, dict(qp_iters=3), "0", 1, "0"),
    "n20-poison": (20, 385, 6, {}, "0", 1, "1"),
    "n12": (12, 130, 3, {}, "0", 1, "0"),
    "n31": (31, 65, 3, {}, "0", 1, "0"),
    "n31-poison": (31, 65, 3, {}, "0", 1, "1"),
    "n19": (19, 65, 3, {}, "0", 1, "0"),
    "n21": (21, 65, 3, {}, "0", 1, "0"),
    "n50": (50, 33, 2, {}, "0", 1, "0"),
    "n50-poison": (50, 33, 2, {}, "0", 1, "1"),
}
# stages per lane and instances per wave (= blocks that walk an instance of their own) of each horizon
LAYOUT = {12: (1, 4), 19: (1, 3), 20: (1, 3), 21: (1, 2), 31: (1, 2), 50: (2, 2)}
N20 = [c for c, v in CASES.items() if v[0] == 20]
POISON = {c: c[:-len("-poison")] for c in CASES if c.endswith("-poison")}


def inputs(N, B):
    sys.path.insert(0, ROOT)
    from bench import SEED, make_inputs
    x0, _, _, sid, traj = make_inputs(B, N, SEED + N)
    return x0, sid, traj


# ------------------------------------------------------------------ the child: device runs only
def child(mode, out_path):
    sys.path.insert(0, ROOT)
    from uclv_qs_pushing_matlab_amd.objects import make_shape
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver
    out = {}
    for name, (N, B, K, opts, fused, parts, poison) in CASES.items():
        if mode == "generic" and N != 20:
            continue
        os.environ["QSP_FUSED_LOOP"] = fused
        os.environ["QSP_DEBUG_POISON"] = poison
        x0, sid, traj = inputs(N, B)
        s = OcpSolver(N=N, batch=B, sqp_iters=K, **opts)
        try:
            s.set_shapes([make_shape(n) for n in NAMES], shape_id=sid)
            s.set_stream_parts(parts)
            s.set_reference_trajectory(traj)
            out[f"{name}/layout"] = np.array(s.layout(), np.int32)
            out[f"{name}/mfma"] = np.int32(s.factor_walk() == MFMA)
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


def reference(N, B, K, opts):
    """The twin's two controller steps (cold, then warm-started from the shifted solution), with the guards on
    the inputs: four shapes in the batch, every QP at the cap in the qp_iters = 3 case, and in the N = 20 case a
    wave whose instances take unequal IPM counts in the warm step's first SQP iteration."""
    key = (N, B, K, tuple(sorted(opts.items())))
    if key in _REF:
        return _REF[key]
    from oracle.oracle import Oracle, make_opts
    twin = Oracle(NAMES, twin=True)
    x0, sid, traj = inputs(N, B)
    assert len(np.unique(sid)) == 4, "the batch mixes the four shapes"
    op = make_opts(N=N, sqp_iters=K, **opts)
    op1 = make_opts(N=N, sqp_iters=1, **opts)
    warm = twin.new_warm(B, N)
    steps, first = [], None
    for step in range(2):
        if step == 1:   # the warm step's first SQP iteration, packed in lane order like every solve's first
            w1 = {k: v.copy() for k, v in warm.items()}
            first = twin.controller_solve(op1, x0, traj, 2, w1, shape_id=sid)["qp_iter"]
        r = twin.controller_solve(op, x0, traj, 1 + step, warm, shape_id=sid)
        r.update(X=warm["X"].copy(), U=warm["U"].copy(), PI=warm["PI"].copy())
        steps.append(r)
    if opts.get("qp_iters") == 3:
        for r in steps:
            assert np.all(r["qp_iter"] == 3 * K), "QPs below the cap"
    elif N == 20:
        G = LAYOUT[N][1]
        q = first[:B // G * G].reshape(-1, G)
        assert np.any(q.min(1) != q.max(1)), "every wave's instances take the same IPM count"
    _REF[key] = steps
    return steps


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Outputs of every case from two fresh processes: 'default' with the library's own dispatch (all cases),
    'generic' with QSP_FIXED_HORIZON=0 (the N = 20 cases)."""
    d = tmp_path_factory.mktemp("walk_stores")
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


@pytest.mark.parametrize("case", list(CASES))
def test_equals_twin(runs, case):
    N, B, K, opts = CASES[case][:4]
    tags = ("default", "generic") if N == 20 else ("default",)
    for step, r in enumerate(reference(N, B, K, opts)):
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
    tags = ("default", "generic") if CASES[case][0] == 20 else ("default",)
    for tag in tags:
        for step in range(2):
            for k in OUT_KEYS:
                same_bytes(runs[tag][f"{case}/{step}/{k}"], runs[tag][f"{POISON[case]}/{step}/{k}"],
                           f"{tag} {case} step {step} {k}")


def test_cases_take_the_walk_and_the_layouts_they_name(runs):
    """Every case factorises on the matrix cores with the stages per lane and instances per wave its row names,
    and the compiled kernel runs at N = 20 only and never under the switch: without this the cases could pass on
    a path that never reaches the stores."""
    for case, (N, *_) in CASES.items():
        S, G = LAYOUT[N]
        lay = tuple(int(v) for v in runs["default"][f"{case}/layout"])
        assert lay[0] == S and 64 // lay[1] == G, (case, lay)
        assert int(runs["default"][f"{case}/mfma"]) == 1, case
        assert int(runs["default"][f"{case}/fixed_horizon"]) == (20 if N == 20 else 0), case
        if N == 20:
            assert int(runs["generic"][f"{case}/mfma"]) == 1 and int(runs["generic"][f"{case}/fixed_horizon"]) == 0, case


if __name__ == "__main__":
    child(sys.argv[1], sys.argv[2])
