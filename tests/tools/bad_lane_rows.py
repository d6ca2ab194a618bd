"""Status of every bad-lane kind (tests/bad_lanes.py) in the literal restatement and in the twin, one row per
kind: controller solves at fixed K and with the merit SQP, the closed loop's two bad lanes step by step, and
the QP level.  `python tests/tools/bad_lane_rows.py [tree]` -- tree: the checkout whose oracle to load (default:
this one), so that the same batches can be put to another commit's build (profiles/bad_lanes/)."""
import os
import sys

import numpy as np

root = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import bad_lanes as bl
from oracle.oracle import Oracle, make_opts
from conftest import straight_traj
NAMES = ("santal", "balea", "montana", "pulirapid")
orc, tw = Oracle(NAMES), Oracle(NAMES, twin=True)
N, S = 20, 1
G = bl.instances_per_wave(N, S)
for nlp, label in ((0, "controller solve, SQP_RTI"), (1, "controller solve, merit SQP")):
    print(f"# {label}, N = {N}, K = 5: kind, rule, literal status/sqp_iter, twin status/sqp_iter")
    op = make_opts(N=N, sqp_iters=5, nlp_mode=nlp)
    for rnd in range(bl.rounds(G)):
        b = bl.ctrl_batch(N, S, seed=3, rnd=rnd)
        w = tw.new_warm(b['B'], N)
        rm = tw.controller_solve(op, b['mixed']['x0'], b['mixed']['traj'], 1, w, shape_id=b['sid'])
        ls, li = bl.literal_controller(orc, op, b['mixed']['x0'], b['mixed']['traj'], 1, b['sid'])
        want = bl.rule_status(b['mixed']['x0'], b['bad'], 0)
        done = set()
        for i in np.flatnonzero(b['bad']):
            k = bl.KINDS[b['kind'][i]].name
            if k in done: continue
            done.add(k)
            flag = '' if (ls[i] == want[i] and rm['status'][i] == want[i]) else '   <-- differs from the rule'
            print(f"{k:16s} rule {want[i]}  literal {ls[i]}/{li[i]}  twin {rm['status'][i]}/{rm['iters'][i]}{flag}")
print("# closed loop, N = 10, T = 6: NaN noise at step 2 of lane a, 1e200 at step 3 of lane b: status per step")
T, N = 6, 10
G = bl.instances_per_wave(N, 1); B = bl.batch_size(G)
mixed, clean, bad, first = bl.closed_loop_noise(T, B, G)
for name, o in (("literal", orc), ("twin", tw)):
    r = o.closed_loop(make_opts(N=N, sqp_iters=5), bl._x0(B, 3), straight_traj(), T, shape_id=np.arange(B) % 4, noise=mixed)
    for lane, t0 in sorted(first.items()):
        print(f"{name:8s} lane {lane} (bad from step {t0}): {r['status'][lane].tolist()}")
print("# qp(), N = 20: kind, literal qp_status/iters, twin qp_status/iters (rule: 1)")
op = make_opts(N=20, sqp_iters=5)
G = bl.instances_per_wave(20, 1)
for rnd in range(bl.rounds(G, bl.QP_KINDS)):
    b = bl.qp_batch(tw, op, rnd=rnd)
    rl = orc.qp(op, *[b['mixed'][k] for k in bl.QP_ARGS]); rt = tw.qp(op, *[b['mixed'][k] for k in bl.QP_ARGS])
    done = set()
    for i in np.flatnonzero(b['bad']):
        k = bl.QP_KINDS[b['kind'][i]].name
        if k in done: continue
        done.add(k)
        print(f"{k:12s} literal {rl['qp_status'][i]}/{rl['iters'][i]}  twin {rt['qp_status'][i]}/{rt['iters'][i]}")
