"""Bad lanes: lanes whose inputs are non-finite or hopeless, mixed into otherwise healthy batches.

A plain module (like manufactured_qp.py) shared by tests/test_bad_lanes.py (the two CPU restatements)
and tests/test_gpu_bad_lanes.py (the device).  It holds the catalogue of bad-lane kinds, their
placement in a batch, the status the rule of include/qsp_nmpc.h (QSP_STATUS_*) gives them -- computed
from the inputs alone -- and a bitwise comparator for the healthy lanes of a mixed batch against the
same batch without its bad lanes.

The rule, "non-finite wins": a lane whose returned iterate (X, U, or the x0 it was given) holds a
non-finite value has status 1; a lane whose iterate stays finite while its QP is infeasible or
diverges has status 4.  Of the kinds below an x0 with a NaN or Inf is the first case; a NaN in the
references (the iterate never moves: finite U, NaN cost), a finite x0 of absurd size and an s_0
outside its bounds are the second.

Placement, with G = instances_per_wave(N, S) instances sharing a wavefront and B = 4 G + 1 lanes:
wave 0 is clean; waves 1 and 2 together have every slot position 0 .. G - 1 bad once (even positions
in wave 1, odd ones in wave 2), so that a bad instance sits next to healthy ones at every position
of the shared matrix-core blocks, LDS record regions and group reductions; wave 3 is bad throughout;
the last, partial wave holds one healthy lane.  That leaves 2 G bad lanes per batch, fewer than the
catalogue has kinds, so the catalogue is dealt over `rounds(G, kinds)` batches: round r carries the
kinds r 2G .. (r + 1) 2G - 1 (cycled to fill the batch), every kind of a round occurs in its batch
(asserted), and the rounds together cover every kind (asserted).
"""
from collections import namedtuple

import numpy as np

NAN, INF = float("nan"), float("inf")
COMP = ("x", "y", "theta", "s")
S_OUT = 0.05      # above uh_s = 0.011 and inside every shape's [-b, b): the wrap leaves it alone

# where: "x0" (component comp), "yref" (stage `stage`: 0 or "mid" = N // 2, component comp of 6),
# "yref_e" (component comp of 4)
Kind = namedtuple("Kind", "name where comp stage value")

X0_NONFINITE = tuple(Kind(f"x0_{COMP[c]}_{tag}", "x0", c, None, v)
                     for c in range(4) for tag, v in (("nan", NAN), ("pinf", INF), ("ninf", -INF)))
X0_HOPELESS = (Kind("x0_x_p1e200", "x0", 0, None, 1e200), Kind("x0_x_m1e200", "x0", 0, None, -1e200),
               Kind("x0_s_out", "x0", 3, None, S_OUT))
YREF_NAN = (Kind("yref0_un_nan", "yref", 4, 0, NAN), Kind("yrefmid_y_nan", "yref", 1, "mid", NAN),
            Kind("yref_e_x_nan", "yref_e", 0, None, NAN))
X0_KINDS = X0_NONFINITE + X0_HOPELESS          # what a shared reference table allows
KINDS = X0_KINDS + YREF_NAN


def instances_per_wave(N, S):
    """qsp_layout.h: one instance owns ceil((N + 1) / S) lanes of a 64-lane wavefront."""
    return 64 // ((N + S) // S)


def batch_size(G):
    return 4 * G + 1


def rounds(G, kinds=KINDS):
    n = -(-len(kinds) // (2 * G))
    seen = set()
    for r in range(n):
        seen |= set(np.unique(placement(G, kinds, r)[1]).tolist())
    assert seen - {-1} == set(range(len(kinds))), "the rounds do not cover the catalogue"
    return n


def placement(G, kinds=KINDS, rnd=0):
    """(bad mask (B,), kind index per lane (B,), -1 on healthy lanes) of round `rnd`."""
    B = batch_size(G)
    bad = np.zeros(B, bool)
    for p in range(G):
        bad[(1 + p % 2) * G + p] = True        # waves 1 and 2: every slot position once
    bad[3 * G:4 * G] = True                    # wave 3: all of it
    assert not bad[:G].any() and not bad[4 * G]
    assert np.all((bad[G:2 * G] | bad[2 * G:3 * G]) & ~(bad[G:2 * G] & bad[2 * G:3 * G]))
    group = list(range(len(kinds)))[rnd * 2 * G:(rnd + 1) * 2 * G]
    assert group, f"round {rnd}: no kinds left"
    kind = np.full(B, -1)
    lanes = np.flatnonzero(bad)
    assert len(lanes) == 2 * G
    for j, i in enumerate(lanes):
        kind[i] = group[j % len(group)]
    assert set(group) <= set(kind[bad].tolist()), "a kind of this round does not occur"
    assert 3 * np.sum(~bad) >= B, "fewer than a third of the lanes are healthy"
    return bad, kind


def rule_status(x0, bad, clean_status):
    """The status by the rule, from the inputs alone: a non-finite x0 gives 1, any other bad lane 4,
    a healthy lane what it has in the clean batch."""
    x0 = np.asarray(x0).reshape(len(bad), -1)
    st = np.where(bad, 4, np.asarray(clean_status))
    return np.where(~np.isfinite(x0).all(1), 1, st).astype(np.int32)


def check_clean(clean_status, bad, merit=False):
    """The healthy lanes must solve in the clean batch, or a test would pass on nothing."""
    st = np.asarray(clean_status)
    ok = np.isin(st, (0, 2)) if merit else st == 0
    assert ok.all(), f"clean batch: lanes {np.flatnonzero(~ok).tolist()} have status {st[~ok].tolist()}"
    assert 3 * np.sum(~np.asarray(bad)) >= len(bad)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def healthy_equal(mixed, clean, bad_mask, what):
    """Every healthy lane (leading axis) of `mixed` has the bits it has in `clean`: floats are compared
    as their 64-bit patterns (so NaN payloads and the sign of zero count), ints as they are.  Raises an
    AssertionError naming the first differing lane."""
    mixed, clean, bad_mask = np.asarray(mixed), np.asarray(clean), np.asarray(bad_mask, bool)
    assert mixed.shape == clean.shape and mixed.dtype == clean.dtype, (what, mixed.shape, clean.shape)
    assert mixed.shape[0] == len(bad_mask), (what, mixed.shape, len(bad_mask))
    assert mixed.dtype == np.float64 or mixed.dtype.kind in "iu", (what, mixed.dtype)
    ne = (_bits(mixed) != _bits(clean)).reshape(len(bad_mask), -1)
    lanes = np.flatnonzero(ne.any(1) & ~bad_mask)
    if len(lanes):
        i = int(lanes[0])
        j = int(np.flatnonzero(ne[i])[0])
        raise AssertionError(f"{what}: {len(lanes)} healthy lanes differ from the clean batch; first lane {i}, entry {j}: "
                             f"mixed {mixed.reshape(len(bad_mask), -1)[i, j]!r} clean "
                             f"{clean.reshape(len(bad_mask), -1)[i, j]!r}")


# ------------------------------------------------------------------ batches
def _x0(B, seed):
    from conftest import config2_x0
    return config2_x0(B, seed)


def _traj(T=60):
    from conftest import straight_traj
    return straight_traj()[:T].copy()


def ocp_batch(N, S, seed=3, kinds=KINDS, rnd=0, index=3):
    """An acados-level batch (x0, yref, yref_e, initial guess X, U) of round `rnd`, mixed and clean.  The
    initial guess is the clean one in both: only x0 and the references carry the bad values."""
    G = instances_per_wave(N, S)
    B = batch_size(G)
    bad, kind = placement(G, kinds, rnd)
    x0 = _x0(B, seed)
    yref = np.broadcast_to(_traj()[None, index:index + N], (B, N, 6)).copy()
    ye = yref[:, -1, :4].copy()
    X = np.repeat(x0[:, None], N + 1, 1)
    U = np.zeros((B, N, 2))
    clean = dict(x0=x0, yref=yref, yref_e=ye)
    mixed = {k: v.copy() for k, v in clean.items()}
    for i in np.flatnonzero(bad):
        k = kinds[kind[i]]
        if k.where == "x0":
            mixed["x0"][i, k.comp] = k.value
        elif k.where == "yref":
            mixed["yref"][i, N // 2 if k.stage == "mid" else k.stage, k.comp] = k.value
        else:
            mixed["yref_e"][i, k.comp] = k.value
    return dict(N=N, B=B, G=G, bad=bad, kind=kind, sid=np.arange(B) % 4, X=X, U=U, clean=clean, mixed=mixed)


def poison(x0, traj, i, k, N, index):
    """Write kind k's value into lane i of a controller-level batch (x0 (B, 4), tables (B, T, 6)) that is
    solved at `index`."""
    if k.where == "x0":
        x0[i, k.comp] = k.value
    elif k.where == "yref":
        traj[i, index - 1 + (N // 2 if k.stage == "mid" else k.stage), k.comp] = k.value
    else:
        traj[i, index - 1 + N - 1, k.comp] = k.value


def ctrl_batch(N, S, seed=3, kinds=KINDS, rnd=0, index=1):
    """A controller-level batch of round `rnd`: x0 and per-lane reference tables (B, T, 6), mixed and
    clean.  Stage k of a solve at `index` reads table row index - 1 + k, the terminal reference row
    index - 1 + N - 1; index_time itself stays the valid `index` on every lane."""
    G = instances_per_wave(N, S)
    B = batch_size(G)
    bad, kind = placement(G, kinds, rnd)
    x0 = _x0(B, seed)
    tab = np.broadcast_to(_traj(index + N + 8)[None], (B, index + N + 8, 6)).copy()
    clean = dict(x0=x0, traj=tab)
    mixed = {k: v.copy() for k, v in clean.items()}
    for i in np.flatnonzero(bad):
        poison(mixed["x0"], mixed["traj"], i, kinds[kind[i]], N, index)
    return dict(N=N, B=B, G=G, bad=bad, kind=kind, sid=np.arange(B) % 4, index=index, clean=clean, mixed=mixed)


def table_groups(traj):
    """Lanes grouped by identical reference table (the literal restatement takes one shared table per
    call): a list of (lane indices, table (T, 6))."""
    traj = np.ascontiguousarray(traj)
    keys = {}
    for i in range(len(traj)):
        keys.setdefault(traj[i].tobytes(), []).append(i)
    return [(np.array(v), traj[v[0]]) for v in keys.values()]


def literal_controller(orc, op, x0, traj, index, sid):
    """One cold-start controller solve of the literal restatement with per-lane tables: one call per
    distinct table.  Returns status, iters (B,)."""
    B = len(x0)
    st, it = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for lanes, tab in table_groups(traj):
        r = orc.controller_solve(op, x0[lanes], tab, index, orc.new_warm(len(lanes), op.N), shape_id=sid[lanes])
        st[lanes], it[lanes] = r["status"], r["iters"]
    return st, it


def closed_loop_noise(T, B, G, seed=1):
    """The closed loop's noise table (T, B, 4), mixed and clean, the two bad lanes and their first bad
    steps (0-based): lane G + 1 gets a NaN in x at step 2 (its plant state, and with it every later x0,
    is NaN: status 1 from step 2 on), lane 2 G + G // 2 gets 1e200 in x at step 3 (finite, hopeless:
    status 4 from step 3 on)."""
    clean = np.random.default_rng(seed).standard_normal((T, B, 4)) * np.array([1e-5, 1e-5, 1e-3, 1e-4])
    mixed = clean.copy()
    a, b = G + 1, 2 * G + G // 2
    mixed[2, a, 0] = NAN
    mixed[3, b, 0] = 1e200
    bad = np.zeros(B, bool)
    bad[[a, b]] = True
    first = {a: 2, b: 3}
    return mixed, clean, bad, first


def closed_loop_rule(clean_status, first, codes):
    """Per-step statuses (B, T) by the rule: the clean run's, and codes[lane] from the lane's first bad
    step on."""
    st = np.array(clean_status, np.int32, copy=True)
    for lane, t0 in first.items():
        st[lane, t0:] = codes[lane]
    return st


# ------------------------------------------------------------------ QPs
# One NaN per bad lane in one of the QP's arrays, at a mid-horizon stage.  H is not among them: only
# the literal restatement reads H lane by lane.  The device and the twin take the weights from lane 0's
# stage-0 and terminal entries of H (ten values; the handle's cost weights are not consulted); the
# device compares every other entry with them and rejects the call when one differs (a NaN differs,
# also from itself), the twin does not compare (include/qsp_nmpc.h, qsp_qp_solve).
# The H cases are tests of their own (test_bad_lanes.test_qp_nan_in_H, test_gpu_bad_lanes.test_qp_solve).
QP_KINDS = tuple(Kind(f"qp_{w}_nan", w, None, "mid", NAN) for w in ("g", "A", "b", "lo", "dx0"))


def qp_batch(orc, op, seed=17, rnd=0):
    """The OCP's Gauss-Newton QPs at perturbed iterates (as test_gpu_twin.test_qp_bit_identical), mixed
    and clean: dicts of A (B, N, 16), B (B, N, 8), b, H, g, lo, hi, act, dx0."""
    from qp_data import build_qp
    N = op.N
    S = op.stages_per_lane if op.stages_per_lane > 0 else (1 if N + 1 <= 32 else 2)
    G = instances_per_wave(N, S)
    nb = batch_size(G)
    bad, kind = placement(G, QP_KINDS, rnd)
    rng = np.random.default_rng(seed)
    x0 = _x0(nb, seed)
    X = np.repeat(x0[:, None], N + 1, 1) + rng.normal(0, 2e-3, (nb, N + 1, 4))
    U = np.stack([rng.uniform(0, 0.03, (nb, N)), rng.uniform(-0.02, 0.02, (nb, N))], 2)
    yref = np.broadcast_to(_traj()[None, :N], (nb, N, 6)).copy()
    A, Bm, b, H, g, lo, hi, act, dx0 = build_qp(orc, op, X, U, yref, yref[:, -1, :4], x0, np.arange(nb) % 4)
    clean = dict(A=A.reshape(nb, N, 16), B=Bm.reshape(nb, N, 8), b=b, H=H, g=g, lo=lo, hi=hi, act=act, dx0=dx0)
    mixed = {k: v.copy() for k, v in clean.items()}
    m = N // 2
    for i in np.flatnonzero(bad):
        w = QP_KINDS[kind[i]].where
        if w == "g":
            mixed["g"][i, 6 * m + 1] = NAN
        elif w == "A":
            mixed["A"][i, m, 3] = NAN          # a03: one of the six entries the structure leaves free
        elif w == "dx0":
            mixed["dx0"][i, 1] = NAN
        else:
            mixed[w][i, m, 1] = NAN
    return dict(N=N, B=nb, G=G, bad=bad, kind=kind, clean=clean, mixed=mixed)


QP_ARGS = ("A", "B", "b", "H", "g", "lo", "hi", "act", "dx0")
